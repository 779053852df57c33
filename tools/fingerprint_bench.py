"""What one fingerprint call costs, against the composition it replaces.  On one MI355X, for the gradient lists of the
C3D and S3D-G pretext models at their real sizes (random values: no step is run):

  (a) one FingerprintSet.run(): rsp_fingerprint, two launches for the whole list;
  (b) the per-parameter ``double().abs().sum()`` stack tools/graph_vs_eager_fullsize.py used before it: three torch launches per tensor;
  (c) the bytes (a) reads over its GPU time, next to the measured HBM copy rate (6.29 TB/s; 8.0 TB/s on paper).  The two model lists
      fit the 256 MiB Infinity Cache, so a 1 GiB list of sixteen tensors is timed as well: that one comes from HBM.

Both bodies in one process, in interleaved blocks of --reps calls after a warm-up; per block the GPU time from a pair of events around the
block and the host issue time from perf_counter around the enqueueing loop (no synchronise inside); median and min-max over the blocks.
The event time of a host-bound body contains its launch gaps: that is what the body costs a step.

    python3 tools/fingerprint_bench.py --out profiles/fingerprint_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_MEASURED_TBS, HBM_PAPER_TBS = 6.29, 8.0


def gradient_list(arch, dev):
    from rspnet_amd.moco import ModelFactory
    cfg = {"model": {"arch": arch}, "moco": {"dim": 128, "k": 16384, "m": 0.999, "t": 0.07, "fc_type": "linear", "diff_speed": [2]}}
    wrapped = ModelFactory(cfg).build_moco_diffloss(device=dev)
    wrapped.module._prepare()      # the flat parameter / gradient buffers, as the first forward builds them
    fl = wrapped.module._flat
    fl.g_flat.normal_()
    names = list(fl.names[:fl.n_trained_params])
    return wrapped, names, [fl.g_flat[o:o + n] for o, n in (fl.offsets[nm] for nm in names)]


def block(body, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        body()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, host * 1e6 / reps      # us per call


def measure(bodies, reps, blocks, warmup):
    for body in bodies.values():
        for _ in range(warmup):
            body()
    torch.cuda.synchronize()
    got = {k: ([], []) for k in bodies}
    for _ in range(blocks):
        for k, body in bodies.items():      # interleaved: every block of one body has a block of the other beside it
            g, h = block(body, reps)
            got[k][0].append(g)
            got[k][1].append(h)
    return got


def fmt(xs):
    return f"{statistics.median(xs):9.1f} ({min(xs):.1f}-{max(xs):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fingerprint_bench: needs the GPU (a time taken elsewhere says nothing)")
    from rspnet_amd import fingerprint as F
    dev = torch.device("cuda", 0)
    lines = [f"fingerprint_bench: {torch.cuda.get_device_name(0)}, {args.blocks} interleaved blocks of {args.reps} calls, us per call: median (min-max)",
             f"{'list':<14}{'tensors':>8}{'MiB':>9}  {'body':<26}{'GPU time':>28}{'host issue time':>28}{'read rate':>12}"]
    cases = [(arch,) + gradient_list(arch, dev)[1:] for arch in ("c3d", "s3dg")]
    big = torch.randn(1 << 28, device=dev)
    cases.append(("1GiB-synthetic", [f"t{i}" for i in range(16)], list(big.view(16, -1).unbind(0))))
    for tag, names, grads in cases:
        nbytes = 4 * sum(g.numel() for g in grads)
        fs = F.FingerprintSet(names, grads)
        bodies = {"(a) FingerprintSet.run()": fs.run}
        if tag != "1GiB-synthetic":
            bodies["(b) double().abs().sum() x n"] = lambda grads=grads: torch.stack([g.double().abs().sum() for g in grads])
        got = measure(bodies, args.reps, args.blocks, args.warmup)
        for k, (g, h) in got.items():
            rate = f"{nbytes / statistics.median(g) / 1e6:8.2f} TB/s" if k.startswith("(a)") else ""
            lines.append(f"{tag:<14}{len(names):>8}{nbytes / 2**20:>9.1f}  {k:<26}{fmt(g):>28}{fmt(h):>28}{rate:>12}")
        # the records are the same bits whichever way they were asked for
        assert torch.equal(fs.run(), fs.run())
    lines.append(f"(c) HBM: {HBM_MEASURED_TBS} TB/s measured float4 copy, {HBM_PAPER_TBS} TB/s on paper; lists below 256 MiB are read from the Infinity Cache "
                 "when they are warm, as here")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
