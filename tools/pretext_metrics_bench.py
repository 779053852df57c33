#!/usr/bin/env python
"""The pretext loop's per-step bookkeeping at the shipped size (B = 32, K = 16384 -> logits (32, 16385)), two bodies run in ONE
process in interleaved blocks (medians over the blocks, with the spread of each):

  "aten"  = what the driver issued per step before rsp_pretext_metrics: accuracy(output[0], topk=(1, 5)), accuracy(cat(ranking
            logits), topk=(1,)), a stack of (loss, loss_A, loss_M, acc1_A) and the add into the running sums;
  "fused" = HipOps.pretext_metrics on the same tensors with a PretextMeters buffer (two kernels, eight meters).

Per body: stream time per call (device events around a block of eagerly issued calls: it contains the idle gaps of a body the host
issues slower than the GPU runs it), host issue time per call (perf_counter around the issue of the block, no sync) and GPU time
per call (the same events around replays of a HIP graph that holds a run of calls: no host in between).  The fused call also
computes acc5_A, both _A_n accuracies and four more meters, which the ATen body never did."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import ops
from rspnet_amd.pretrain import PretextMeters, accuracy, pretext_accuracy

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--k", type=int, default=16384)
ap.add_argument("--calls", type=int, default=200, help="calls per block")
ap.add_argument("--blocks", type=int, default=7, help="interleaved blocks per body")
args = ap.parse_args()
assert torch.cuda.is_available(), "pretext_metrics_bench needs a GPU"
dev = torch.device("cuda", 0)
be = ops.backend()
assert be.name == "hip"
B, K1 = args.batch, args.k + 1
g = torch.Generator(device=dev).manual_seed(0)
output = (torch.randn(B, K1, device=dev, generator=g), torch.randn(B, K1, device=dev, generator=g))
ranking = (torch.randn(B, 1, device=dev, generator=g), torch.randn(B, 1, device=dev, generator=g))
losses = torch.rand(3, device=dev, generator=g)
loss, loss_A, loss_M = losses[0], losses[1], losses[2]
target = torch.zeros(B, dtype=torch.long, device=dev)
sums = torch.zeros(4, device=dev)
meters = PretextMeters(dev)


def aten():
    global sums
    acc1_A, acc5_A = accuracy(output[0], target, topk=(1, 5))
    acc1_M, = accuracy(torch.cat(ranking, dim=1), target, topk=(1,))
    sums += torch.stack([loss.detach(), loss_A, loss_M, acc1_A])


def fused():
    be.pretext_metrics(output[0], output[1], ranking[0], ranking[1], losses, meters.buf)


def block(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    host = time.perf_counter() - h0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls * 1e3, host / args.calls * 1e6      # both in us per call


GRAPH_CALLS, GRAPH_REPLAYS = 20, 10


def graphed(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(GRAPH_CALLS):
            fn()
    graph.replay()
    return graph


def graph_block(graph):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(GRAPH_REPLAYS):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (GRAPH_CALLS * GRAPH_REPLAYS) * 1e3


# the two bodies agree on what both compute
want = pretext_accuracy(output, ranking)
got = be.pretext_metrics(output[0], output[1], ranking[0], ranking[1], losses)
a1, a5 = accuracy(output[0], target, topk=(1, 5))
assert torch.equal(got, want) and float(got[0]) == float(a1) and float(got[1]) == float(a5)

bodies = {"aten": aten, "fused": fused}
for fn in bodies.values():
    for _ in range(20):
        fn()
graphs = {k: graphed(fn) for k, fn in bodies.items()}
res = {k: [] for k in bodies}
for _ in range(args.blocks):
    for k, fn in bodies.items():
        res[k].append(block(fn) + (graph_block(graphs[k]),))
med = {}
for k, r in res.items():
    stream, host, gpu = [a for a, _, _ in r], [b for _, b, _ in r], [c for _, _, c in r]
    med[k] = (statistics.median(gpu), statistics.median(host), statistics.median(stream))
    print(f"B={B} K1={K1} {k:5s}: GPU time per call median {med[k][0]:.1f} us (min {min(gpu):.1f}, max {max(gpu):.1f}; graph of "
          f"{GRAPH_CALLS} calls x {GRAPH_REPLAYS} replays); host issue per call median {med[k][1]:.1f} us (min {min(host):.1f}, max "
          f"{max(host):.1f}); stream time per eager call median {med[k][2]:.1f} us (min {min(stream):.1f}, max {max(stream):.1f}); "
          f"{args.blocks} blocks x {args.calls} calls")
print(f"fused - aten: GPU {med['fused'][0] - med['aten'][0]:+.1f} us, host {med['fused'][1] - med['aten'][1]:+.1f} us per call")
