#!/usr/bin/env python
"""Eval-mode (one-pass) vs train-mode (reduce + apply) BatchNorm backward, timed in ONE process.

    python tools/bn_bwd_bench.py [--blocks 7] [--iters 20] [--out profiles/bn_eval_bwd_bench.txt]

The train-mode pair (rsp_bn_act_pool_bwd) is the yardstick: the one-pass op moves strictly fewer bytes, so on every geometry it
must not be slower.  Geometries: the BatchNorm units of C3D conv2 .. conv5b and of R3D-18 layer1 .. layer4 at B = 32, 16 x 112^2
clips.  The two ops alternate in blocks of `iters` calls (device events around each block); reported per op: the median block and
the min-max over the blocks, achieved GB/s from the byte counts the ops log for the roofline pass (ops.HipOps._log_hbm), and the
ratio of the medians.  Exit status 1 if a geometry loses (its numbers are in the table)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import ops
from rspnet_amd.ops import PoolGeom

# name, N, D, H, W, C, pool window (== stride), residual
GEOMS = [
    ("c3d conv2 +pool222", 32, 16, 56, 56, 128, (2, 2, 2), False),
    ("c3d conv3a", 32, 8, 28, 28, 256, (1, 1, 1), False),
    ("c3d conv3b +pool222", 32, 8, 28, 28, 256, (2, 2, 2), False),
    ("c3d conv4a", 32, 4, 14, 14, 512, (1, 1, 1), False),
    ("c3d conv4b +pool222", 32, 4, 14, 14, 512, (2, 2, 2), False),
    ("c3d conv5a / conv5b", 32, 2, 7, 7, 512, (1, 1, 1), False),
    ("r3d18 layer1 conv1", 32, 8, 28, 28, 64, (1, 1, 1), False),
    ("r3d18 layer1 conv2 +res", 32, 8, 28, 28, 64, (1, 1, 1), True),
    ("r3d18 layer2 conv1", 32, 4, 14, 14, 128, (1, 1, 1), False),
    ("r3d18 layer2 conv2 +res", 32, 4, 14, 14, 128, (1, 1, 1), True),
    ("r3d18 layer3 conv1", 32, 2, 7, 7, 256, (1, 1, 1), False),
    ("r3d18 layer3 conv2 +res", 32, 2, 7, 7, 256, (1, 1, 1), True),
    ("r3d18 layer4 conv1", 32, 1, 4, 4, 512, (1, 1, 1), False),
    ("r3d18 layer4 conv2 +res", 32, 1, 4, 4, 512, (1, 1, 1), True),
]


def block_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def logged_bytes(be, fn):
    be.event_log, be.hbm_log = [], []
    fn()
    torch.cuda.synchronize()
    n = sum(rec[1] for rec in be.hbm_log)
    be.event_log = be.hbm_log = None
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.blocks >= 5
    be = ops.backend()
    assert be.name == "hip"
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.blocks} interleaved blocks of {args.iters} calls; ms = median block [min-max]; "
             "GB/s = logged algorithmic bytes / median",
             f"{'geometry':26s} {'train pair ms':>24s} {'GB/s':>6s} {'one pass ms':>24s} {'GB/s':>6s} {'no sums ms':>10s} {'ratio':>6s}"]
    lost = []
    for name, N, D, H, W, C, k, use_res in GEOMS:
        g = torch.Generator(device=dev).manual_seed(1)
        pg = PoolGeom(N, D, H, W, C, k, k, (0, 0, 0))
        y = torch.randn(N, D, H, W, C, device=dev, generator=g)
        res = torch.randn(N, D, H, W, C, device=dev, generator=g) if use_res else None
        ss = torch.stack([torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g) * 0.1])
        mi = torch.stack([torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5])
        gamma = torch.rand(C, device=dev, generator=g) + 0.5
        do, ho, wo = pg.out_dims
        dout = torch.randn(N, do, ho, wo, C, device=dev, generator=g)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        dy = torch.empty_like(y)
        train = lambda: be.bn_act_pool_bwd(pg, y, res, dout, gamma, mi, ss, True, use_res, dg, db, dy_out=dy)
        one = lambda: be.bn_eval_act_pool_bwd(pg, y, res, dout, mi, ss, True, use_res, dg, db, dy_out=dy)
        nosum = lambda: be.bn_eval_act_pool_bwd(pg, y, res, dout, mi, ss, True, use_res, None, None, dy_out=dy)
        bytes_t, bytes_e = logged_bytes(be, train), logged_bytes(be, one)
        for fn in (train, one, nosum):          # warm-up of every shape the timed window uses
            block_ms(fn, 3)
        t, e, z = [], [], []
        for _ in range(args.blocks):
            t.append(block_ms(train, args.iters))
            e.append(block_ms(one, args.iters))
            z.append(block_ms(nosum, args.iters))
        mt, me, mz = statistics.median(t), statistics.median(e), statistics.median(z)
        ratio = me / mt
        if ratio > 1.0:
            lost.append(name)
        lines.append(f"{name:26s} {mt:8.4f} [{min(t):.4f}-{max(t):.4f}] {bytes_t / mt / 1e6:6.0f} "
                     f"{me:8.4f} [{min(e):.4f}-{max(e):.4f}] {bytes_e / me / 1e6:6.0f} {mz:10.4f} {ratio:6.3f}")
        print(lines[-1], flush=True)
        del y, res, dout, dy
    lines.append("# one pass not slower than the train-mode pair on every geometry: " + ("yes" if not lost else "NO: " + ", ".join(lost)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
