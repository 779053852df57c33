#!/usr/bin/env python
"""Fine-tune step throughput: MultiTaskWrapper(finetune=True) train step (forward + CrossEntropyLoss + backward
+ torch SGD) and eval-mode forward at the pretext geometry, B=32 clips of 3x16x112x112, 101 classes (UCF-101), one MI355X.
Conv FLOPs per clip: train 3F - F_first, eval F (C3D F = 76.99 GF, first conv 2.08).

--loop adds the train step with everything the fine-tune loop does behind the logits, in two bodies run in ONE process in
interleaved blocks (medians over the blocks, with the spread of each): "unfused" = the reference loop body as it stands (model +
nn.CrossEntropyLoss + torch accuracy(topk=(1, 5)) + three tensor meters + torch SGD), "fused" = FusedCrossEntropy + Meters
(rsp_xent_metrics) + torch SGD.  Per body also the host time per step: perf_counter around the issue of a step, no sync."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd.finetune import train_step, validate_step
from rspnet_amd.models import ModelFactory

GF = {"c3d": (76.99, 2.08), "resnet18": (16.62, 6.61), "r2plus1d-vcop": (42.72, 1.22), "s3dg": (34.07, 1.89)}
ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="c3d", choices=sorted(GF))
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--loop", action="store_true", help="also time the unfused / fused loop bodies")
ap.add_argument("--blocks", type=int, default=5, help="--loop: interleaved blocks per body")
args = ap.parse_args()
dev = torch.device("cuda", 0)
hw = 224 if args.arch == "s3dg" else 112
model = ModelFactory({"model": {"arch": args.arch}, "dataset": {"num_classes": 101}}).build_multitask_wrapper(0)
crit = torch.nn.CrossEntropyLoss()
opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(args.batch, 3, 16, hw, hw, device=dev, generator=g)
y = torch.randint(0, 101, (args.batch,), device=dev, generator=g)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps


model.train()
t_train = timed(lambda: train_step(model, crit, opt, x, y))
model.eval()
t_eval = timed(lambda: validate_step(model, crit, x, y))
F, F1 = GF[args.arch]
print(f"{args.arch} B={args.batch} {hw}x{hw}: train step {t_train * 1e3:.1f} ms = {args.batch / t_train:.0f} clips/s "
      f"({args.batch * (3 * F - F1) / t_train / 1e3:.1f} conv TFLOP/s); eval forward {t_eval * 1e3:.1f} ms = {args.batch / t_eval:.0f} clips/s "
      f"({args.batch * F / t_eval / 1e3:.1f} conv TFLOP/s)")


if args.loop:
    import statistics

    from rspnet_amd.finetune import FusedCrossEntropy, Meters
    from rspnet_amd.pretrain import accuracy

    class TensorMeter:      # framework/meters/average.py: three device scalars, updated in place
        def __init__(self):
            self.val = torch.tensor(0, dtype=torch.float, device=dev)
            self.sum = torch.tensor(0, dtype=torch.float, device=dev)
            self.count = torch.tensor(0, dtype=torch.int, device=dev)

        @torch.no_grad()
        def update(self, val, n=1):
            self.val = val
            self.sum += val * n
            self.count += n

    tmeters = [TensorMeter() for _ in range(3)]
    fused, fmeters = FusedCrossEntropy(), Meters(dev)
    model.train()

    def unfused_step():
        output = model(x)
        loss = crit(output, y)
        acc1, acc5 = accuracy(output, y, topk=(1, 5))
        tmeters[1].update(acc1, args.batch)
        tmeters[2].update(acc5, args.batch)
        tmeters[0].update(loss.detach(), args.batch)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def fused_step():
        loss = fused(model(x), y, n_crop=1, valid=args.batch, meters=fmeters)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def block(fn):
        torch.cuda.synchronize()
        host, t0 = 0.0, time.perf_counter()
        for _ in range(args.steps):
            h0 = time.perf_counter()
            fn()
            host += time.perf_counter() - h0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, host / args.steps * 1e3

    bodies = {"unfused": unfused_step, "fused": fused_step}
    for fn in bodies.values():
        for _ in range(3):
            fn()
    res = {k: [] for k in bodies}
    for _ in range(args.blocks):
        for k, fn in bodies.items():
            res[k].append(block(fn))
    med = {}
    for k, r in res.items():
        step, host = [a for a, _ in r], [b for _, b in r]
        med[k] = (statistics.median(step), statistics.median(host))
        print(f"{args.arch} B={args.batch} loop body {k:8s}: step median {med[k][0]:.3f} ms (min {min(step):.3f}, max {max(step):.3f}); "
              f"host issue median {med[k][1]:.3f} ms (min {min(host):.3f}, max {max(host):.3f}); "
              f"{args.blocks} blocks x {args.steps} steps")
    print(f"{args.arch} fused - unfused: step {med['fused'][0] - med['unfused'][0]:+.3f} ms, "
          f"host {med['fused'][1] - med['unfused'][1]:+.3f} ms")
