#!/usr/bin/env python
"""Time of the label-free representation statistics (rsp_repr_stats: pair sums, Gram matrix and column sums, one call) on one MI355X,
at the pretext queue's size and at the UCF-101 split-1 feature bank with two feature widths; alongside, on the same inputs and in the
same process, the composition of the same sums from torch ops (it stores the N x N matrix; a measurement baseline, not a product
path) and the call without the Gram matrix.  Device events around one call each (knn_bench's timer), every shape and every body
warmed first, the bodies interleaved repeat by repeat so that they see the same state of the machine; median (min - max) ms.  The
arithmetic beside each time is the algorithm's: N^2 D FLOP for the pairs (each pair once, 2 FLOP per k) and 2 N D^2 for the Gram
matrix as launched (both triangles), over the whole call's time -- a call rate, not a kernel's share of peak.

    python tools/repr_bench.py [--repeats 21] [--out profiles/repr_stats_bench.txt] [--resources FILE]

--resources: a text file with the compiler's resource report of the kernels, copied into the output.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from knn_bench import timed_ms
from rspnet_amd import ops

SHAPES = [(16384, 128), (9537, 512), (9537, 2048)]      # N, D
PEAK_TFLOPS = 157.3                                     # fp32 MFMA


def torch_composition(x, t):
    """The same three pair sums, Gram matrix and column sums from torch ops in fp32; the N x N matrix is stored."""
    ss = (x * x).sum(dim=1)
    xh = x * (1.0 / ss.sqrt())[:, None]
    s = xh @ xh.t()
    keep = torch.ones_like(s, dtype=torch.bool).triu_(1)
    e = torch.where(keep, torch.exp(2.0 * t * (s - 1.0)), torch.zeros_like(s))
    sk = torch.where(keep, s, torch.zeros_like(s))
    return e.sum(dtype=torch.float64), sk.sum(dtype=torch.float64), (sk * sk).sum(dtype=torch.float64), xh.t() @ xh, xh.sum(dim=0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats: a median of at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("repr_bench: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    be = ops.backend()
    lines = [f"repr_bench: {torch.cuda.get_device_name(0)}, {args.repeats} interleaved repeats after {args.warmup} warm-up calls, "
             f"ms per call: median (min - max)"]
    t = 2.0
    for N, D in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(N, D, device=dev, generator=gen) + 0.3 * torch.randn(1, D, device=dev, generator=gen)
        bodies = (("rsp_repr_stats", lambda: be.repr_stats(x, t)),
                  ("rsp_repr_stats, no Gram", lambda: be.repr_stats(x, t, want_gram=False)),
                  ("torch composition", lambda: torch_composition(x, t)))
        for _, fn in bodies:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in bodies}
        for _ in range(args.repeats):
            for name, fn in bodies:
                times[name].append(timed_ms(fn))
        res = be.repr_stats(x, t)
        pe, pc, pc2, gram, colsum = torch_composition(x, t)
        got = torch.frombuffer(bytearray(res.sums.cpu().numpy().tobytes()[:24]), dtype=torch.float64)
        agree = max(abs(float(got[0]) - float(pe)) / float(pe), abs(float(got[2]) - float(pc2)) / float(pc2),
                    float((res.gram - gram.double()).abs().max() / gram.abs().max()))
        flop_pair, flop_gram = float(N) * N * D, 2.0 * N * D * D
        lines.append(f"N {N} x D {D}: pairs {flop_pair:.2e} FLOP + Gram {flop_gram:.2e} FLOP = "
                     f"{1e3 * (flop_pair + flop_gram) / (PEAK_TFLOPS * 1e12):.3f} ms at the fp32-MFMA peak of {PEAK_TFLOPS} TFLOP/s "
                     f"(largest relative difference to the torch composition {agree:.1e})")
        for name, _ in bodies:
            v = times[name]
            flop = flop_pair + (flop_gram if name != "rsp_repr_stats, no Gram" else 0.0)
            lines.append(f"  {name:<26}{statistics.median(v):10.3f} ({min(v):.3f} - {max(v):.3f})"
                         f"   {flop / (1e9 * statistics.median(v)):8.1f} TFLOP/s over the call")
        del x, gram
        torch.cuda.empty_cache()
    if args.resources and os.path.exists(args.resources):
        lines.append("compiler resource report (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage):")
        lines.extend("  " + l.rstrip() for l in open(args.resources))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
