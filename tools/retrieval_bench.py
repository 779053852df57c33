#!/usr/bin/env python
"""Retrieval throughput on one MI355X: feature extraction (Engine.features: get_feature + spatial mean + crop average) per arch at
the reference's retrieval config (10 crops, batch 8, 16 x 112^2; S3D-G 16 x 224^2), and the fused cosine top-k search
(rsp_cosine_topk, k = 50) at the UCF-101 split-1 size and at a large gallery.  For the search, an unfused torch.mm + torch.topk
run on the same inputs is timed alongside, interleaved repeat by repeat: a measurement baseline only (not a product path).
Share of peak: 2 Nq Ng D FLOP over the 157.3 TF fp32-MFMA peak."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import ops
from rspnet_amd.models import ModelFactory
from rspnet_amd.retrieval import Engine

PEAK = 157.3e12
ap = argparse.ArgumentParser()
ap.add_argument("--archs", default="c3d,resnet18,r2plus1d-vcop,s3dg")
ap.add_argument("--batches", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sizes", default="3783x9537x512,20000x200000x512")
ap.add_argument("--skip-extract", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
out = {"extract": {}, "search": {}}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


if not args.skip_extract:
    for arch in args.archs.split(","):
        hw = 224 if arch == "s3dg" else 112
        model = ModelFactory({"model": {"arch": arch}, "dataset": {"num_classes": 101}}).build(0)
        eng = Engine(model, n_crop=10, device=dev)
        model.eval()
        clip = torch.randn(8, 3, 160, hw, hw, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        for _ in range(2):
            eng.features(clip)
        torch.cuda.synchronize()
        t = timed(lambda: [eng.features(clip) for _ in range(args.batches)])
        rate = args.batches * 8 * 10 / t
        out["extract"][arch] = {"crops_per_s": rate, "videos_per_s": rate / 10, "hw": hw}
        print(f"extract {arch}: {rate:.1f} crop clips/s ({rate / 10:.1f} videos/s, 16x{hw}^2, batch 8 x 10 crops)", flush=True)
        del model, eng, clip
        torch.cuda.empty_cache()

be = ops.backend()
for size in args.sizes.split(","):
    Nq, Ng, D = (int(v) for v in size.split("x"))
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn(Nq, D, device=dev, generator=g)
    gal = torch.randn(Ng, D, device=dev, generator=g)
    flop = 2.0 * Nq * Ng * D

    def fused():
        be.cosine_topk(q, gal, 50)

    def unfused():
        qn = q / q.norm(dim=1, keepdim=True)
        gn = gal / gal.norm(dim=1, keepdim=True)
        torch.topk(torch.mm(qn, gn.t()), 50, dim=1)

    for fn in (fused, unfused):
        fn()
    torch.cuda.synchronize()
    tf, tu = [], []
    for _ in range(args.repeats):         # interleaved: both see the same box state
        tf.append(timed(fused))
        tu.append(timed(unfused))
        torch.cuda.empty_cache()
    rec = {"fused_ms": [x * 1e3 for x in tf], "mm_topk_ms": [x * 1e3 for x in tu],
           "fused_median_ms": statistics.median(tf) * 1e3, "mm_topk_median_ms": statistics.median(tu) * 1e3,
           "fused_peak_frac": flop / statistics.median(tf) / PEAK, "mm_topk_peak_frac": flop / statistics.median(tu) / PEAK,
           "splits": int(be.lib.rsp_cosine_topk_splits(Nq, Ng, 0))}
    out["search"][size] = rec
    print(f"search {size}: fused {rec['fused_median_ms']:.2f} ms (min {min(tf) * 1e3:.2f}, max {max(tf) * 1e3:.2f}; "
          f"{rec['fused_peak_frac'] * 100:.1f} % of fp32 MFMA peak), mm+topk {rec['mm_topk_median_ms']:.2f} ms "
          f"(min {min(tu) * 1e3:.2f}, max {max(tu) * 1e3:.2f}; {rec['mm_topk_peak_frac'] * 100:.1f} %)", flush=True)
    del q, gal
    torch.cuda.empty_cache()
print(json.dumps(out))
