#!/usr/bin/env python
"""Time of the linear probe on one MI355X: 100 full-batch steps of rsp_linear_probe_fit from zeros, then rsp_linear_probe_logits and
rsp_xent_metrics on the test rows, at the UCF-101 split-1 size (9 537 x 512 -> 101, 3 783 test rows) and at 16 384 x 2 048 -> 400;
alongside, on the same inputs and in the same process, the same call with the general (four launches per step) path forced, and the
composition of the same rule from torch ops (rspnet_amd.linear_probe._probe_torch: the library GEMM, a host loop; a measurement
baseline, not a product path).  Device events around one call each, every shape and every body warmed first, the three bodies
interleaved repeat by repeat so that they see the same state of the machine; median (min - max) ms, and the achieved TF/s of the
whole call against 2 * (2 N D C) FLOP per step (the evaluation's share of the time is counted, its FLOP are not).

    python tools/probe_bench.py [--repeats 21] [--out profiles/probe_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from rspnet_amd import linear_probe, ops

SHAPES = [(9537, 3783, 512, 101), (16384, 4096, 2048, 400)]      # N, test rows, D, classes
STEPS = 100


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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats < 20:
        ap.error("--repeats: a median of at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("probe_bench: no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    be = ops.backend()
    lines = [f"probe_bench: {torch.cuda.get_device_name(0)}, {STEPS} full-batch steps + evaluation per call, {args.repeats} interleaved "
             f"repeats after {args.warmup} warm-up calls, ms per call: median (min - max), TF/s at the median"]
    for N, Nt, D, C in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(1)
        mu = torch.randn(C, D, device=dev, generator=gen)
        y = torch.randint(0, C, (N,), device=dev, generator=gen)
        yt = torch.randint(0, C, (Nt,), device=dev, generator=gen)
        x = 0.15 * mu[y] + torch.randn(N, D, device=dev, generator=gen)
        xt = 0.15 * mu[yt] + torch.randn(Nt, D, device=dev, generator=gen)
        lr = torch.from_numpy(linear_probe.lr_schedule(0.125, STEPS)).to(dev)
        w, b, mom = torch.zeros(C, D, device=dev), torch.zeros(C, device=dev), torch.zeros(C * D + C, device=dev)
        out = {}

        def hip(name, general):
            def body():
                if general:
                    os.environ["RSP_PROBE_GENERAL"] = "1"
                try:
                    w.zero_(), b.zero_(), mom.zero_()
                    trace, _ = be.linear_probe_fit(x, y, w, b, mom, lr, STEPS, N)
                    z = be.linear_probe_logits(xt, w, b)
                    _, loss, acc, _ = be.xent_metrics(z, yt, want_grad=False)
                finally:
                    os.environ.pop("RSP_PROBE_GENERAL", None)
                out[name] = (trace, loss, acc)
            return body

        def composed():
            w.zero_(), b.zero_(), mom.zero_()
            trace, _ = linear_probe._probe_torch(x, y, w, b, mom, lr, STEPS, N)
            z = linear_probe._logits_torch(xt, w, b, True, 8.0)
            _, loss, acc, _ = be.xent_metrics(z, yt, want_grad=False)
            out["torch"] = (trace, loss, acc)

        fused = C <= 256
        bodies = ((f"rsp_linear_probe_fit ({'fused: 3' if fused else 'general: 4'} launches/step)", hip("hip", False)),
                  ("general path forced (4 launches/step)", hip("general", True)),
                  ("torch composition (host loop, >= 12 ops/step)", composed))
        for _, fn in bodies:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in bodies}
        for _ in range(args.repeats):
            for name, fn in bodies:
                times[name].append(timed_ms(fn))
        torch.cuda.synchronize()
        acc = {k: [float(v) for v in out[k][2].cpu()] for k in out}
        gap = {k: float((out[k][0] - out["torch"][0]).abs().max()) for k in ("hip", "general")}
        lines.append(f"N {N} x D {D} -> {C} classes, {Nt} test rows (final train loss {float(out['hip'][0][-1]):.4f}; test Acc@1 "
                     f"{acc['hip'][0]:.2f} / general {acc['general'][0]:.2f} / torch {acc['torch'][0]:.2f}; max |loss_trace - torch's| "
                     f"{gap['hip']:.1e} / general {gap['general']:.1e})")
        flop = STEPS * 2.0 * (2.0 * N * D * C)
        for name, _ in bodies:
            t = times[name]
            med = statistics.median(t)
            lines.append(f"  {name:<50}{med:10.3f} ({min(t):.3f} - {max(t):.3f}){flop / (med * 1e-3) / 1e12:8.1f} TF/s")
        del x, xt, mu
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
