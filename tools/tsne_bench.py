#!/usr/bin/env python
"""Time of the embedding maps on one MI355X: rsp_tsne_affinities (one call) and a 100-iteration rsp_tsne_fit (one call, three launches
per iteration, the N x N matrices of the map never stored) at the UCF-101 split-1 train size (9 537 x 512) and at the MoCo queue's
(16 384 x 128), perplexity 30; alongside, on the same inputs and in the same process, the same rule composed from torch ops
(rspnet_amd.tsne.affinities_torch / step_torch: it stores the N x N x 2 difference tensor and several N x N temporaries per iteration
-- a measurement baseline, and what a backend without the entry points runs).  Device events around one call
each (cluster_bench's helper), every body warmed first, the two bodies interleaved repeat by repeat; median (min - max) ms per call,
and next to it the host's issue time.

    python tools/tsne_bench.py [--repeats 7] [--out profiles/tsne_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from cluster_bench import timed
from rspnet_amd import ops, tsne

SHAPES = [(9537, 512, 101), (16384, 128, 256)]      # N, D, classes of the synthetic rows
ITERS, PERPLEXITY = 100, 30.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    be = ops.backend()
    lines = [f"tsne_bench: {torch.cuda.get_device_name(0)}, perplexity {PERPLEXITY:g}, {ITERS} iterations per fit call, {args.repeats} "
             f"interleaved repeats after {args.warmup} warm-up calls, ms per call: device median (min - max) | host issue median"]
    for N, D, C in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        mu = torch.randn(C, D, device=dev, generator=gen)
        lab = torch.randint(0, C, (N,), device=dev, generator=gen)
        x = 0.15 * mu[lab] + torch.randn(N, D, device=dev, generator=gen)
        y0 = tsne.initial_map(x, 0).to(dev)
        sched_np = tsne.schedule(ITERS, max(N / 12.0 / 4.0, 50.0))
        sched = torch.from_numpy(sched_np).to(dev)
        steps = [tuple(float(v) for v in row[:3]) for row in sched_np]
        out = {}

        def aff_hip():
            out["aff"] = be.tsne_affinities(x, PERPLEXITY)

        def aff_torch():
            out["aff_t"] = tsne.affinities_torch(x, PERPLEXITY)

        def fit_hip():
            y, inc, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
            out["kl"] = be.tsne_fit(out["aff"], sched, 0, ITERS, y, inc, gains)

        def fit_torch():
            p, plogp = out["aff_t"][3], out["aff_t"][4]
            y, inc, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
            for lr, mom, ex in steps:
                out["kl_t"] = tsne.step_torch(p, plogp, y, inc, gains, lr, mom, ex)[1]

        groups = ((("rsp_tsne_affinities (one call, 6 launches)", aff_hip), ("torch composition (~10 ops x 64 bisection steps)", aff_torch)),
                  ((f"rsp_tsne_fit ({ITERS} iterations, 3 launches each)", fit_hip), ("torch composition (host loop, ~25 ops/iteration)", fit_torch)))
        lines.append(f"N {N} x D {D}")
        for bodies in groups:
            for _, fn in bodies:
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in bodies}
            for _ in range(args.repeats):
                for name, fn in bodies:
                    times[name].append(timed(fn))
            torch.cuda.synchronize()
            for name, _ in bodies:
                d, h = [v[0] for v in times[name]], [v[1] for v in times[name]]
                lines.append(f"  {name:<56}{statistics.median(d):11.3f} ({min(d):.3f} - {max(d):.3f}) | {statistics.median(h):9.3f}")
        info = tsne.read_info(out["aff"].info)
        lines.append(f"  (sum p {info['psum']:.6f} against {out['aff_t'][5]:.6f}; KL before iteration {ITERS - 1}: {float(out['kl'][-1]):.5f} "
                     f"against {float(out['kl_t']):.5f})")
        out.clear()
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
