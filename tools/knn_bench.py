#!/usr/bin/env python
"""Time of the weighted kNN classifier (rsp_knn_classify, k = 200) on one MI355X, at the UCF-101 split-1 size and at a large bank;
alongside, on the same inputs and in the same process, the retrieval search (rsp_cosine_topk, k = 50: what the wider per-query list
and the vote cost on top of it) and the composition of the same rule from torch ops (rspnet_amd.knn._knn_torch: it stores the
Nq x Ng matrix; a measurement baseline, not a product path).  Device events around one call each, every shape and every body warmed
first, the three bodies interleaved repeat by repeat so that they see the same state of the machine; median (min - max) ms.

    python tools/knn_bench.py [--repeats 21] [--out profiles/knn_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import knn, ops

SHAPES = [(3783, 9537, 512, 200, 101), (4096, 65536, 512, 200, 400)]      # Nq, Ng, D, k, classes


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats: a median of at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    be = ops.backend()
    lines = [f"knn_bench: {torch.cuda.get_device_name(0)}, {args.repeats} interleaved repeats after {args.warmup} warm-up calls, "
             f"ms per call: median (min - max)"]
    for Nq, Ng, D, k, C in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        mu = torch.randn(C, D, device=dev, generator=gen)
        yq = torch.randint(0, C, (Nq,), device=dev, generator=gen)
        yg = torch.randint(0, C, (Ng,), device=dev, generator=gen)
        q = 0.15 * mu[yq] + torch.randn(Nq, D, device=dev, generator=gen)
        g = 0.15 * mu[yg] + torch.randn(Ng, D, device=dev, generator=gen)
        bodies = (("rsp_knn_classify k=200", lambda: be.knn_classify(q, g, yg, k, 0.07, C, y_q=yq)),
                  ("rsp_cosine_topk k=50", lambda: be.cosine_topk(q, g, 50)),
                  ("torch composition k=200", lambda: knn._knn_torch(q, yq, g, yg, k, 0.07, C)))
        for _, fn in bodies:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in bodies}
        for _ in range(args.repeats):
            for name, fn in bodies:
                times[name].append(timed_ms(fn))
        res = be.knn_classify(q, g, yg, k, 0.07, C, y_q=yq)
        _, trank, _ = knn._knn_torch(q, yq, g, yg, k, 0.07, C)
        agree = float((res.rank.to(torch.int64) == trank).float().mean())
        h1, h5 = res.hits.cpu().tolist()
        lines.append(f"Nq {Nq} x Ng {Ng} x D {D}, {C} classes, {int(be.lib.rsp_cosine_topk_splits(Nq, Ng, 0))} gallery splits "
                     f"(Acc@1 {100.0 * h1 / Nq:.2f}, Acc@5 {100.0 * h5 / Nq:.2f}; ranks equal to the torch composition's on "
                     f"{100.0 * agree:.2f} % of the queries)")
        for name, _ in bodies:
            t = times[name]
            lines.append(f"  {name:<26}{statistics.median(t):10.3f} ({min(t):.3f} - {max(t):.3f})")
        del q, g, mu
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
