"""Generate tests/golden/finetune_frozen_bn_<arch>.npz: the REFERENCE's MultiTaskWrapper(finetune=True) in EVAL mode (BatchNorm on
its running statistics), forward + CrossEntropyLoss + backward.  Build machine only (needs the reference checkout that
oracle.ref_harness imports).  TEST INFRASTRUCTURE ONLY.

    python tools/gen_golden_frozen_bn.py [arch ...]

Cases, sizes, seed screen (checker-backend gradient error, ReLU / pool margin) and summary format are those of
oracle/gen_golden_finetune.py; the guard band is computed on the EVAL forward, whose ReLU decisions differ from the train-mode
fixture's.  The state spec is the train-mode fixture's (tests/golden/finetune_spec_<arch>.json: same model).

The gradient gate comes from the reference itself: the same model, state and inputs are evaluated once more in fp64, and the worst
per-parameter relative L2 distance between the fp32 and the fp64 gradients is stored as `floor` in the meta.  The tests hold the
product to three such floors, never below 3e-3."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import guard
from oracle import portable as P
from oracle import ref_harness as R
from oracle import restatement as S
from oracle.gen_golden_finetune import CASES, SEED_GATE

BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def run_reference_eval(model, state, x, target, dtype=torch.float32):
    """Eval-mode forward + CrossEntropyLoss + backward of the reference wrapper; asserts that no BatchNorm buffer moved."""
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    model.to(dtype)
    model.eval()
    model.zero_grad()
    handles, margins = R.register_margin_hooks(model)
    logits = model(torch.from_numpy(x).to(dtype))
    for h in handles:
        h.remove()
    loss = torch.nn.CrossEntropyLoss()(logits, torch.from_numpy(target))
    loss.backward()
    grads = {n: (None if p.grad is None else p.grad.detach().numpy().copy()) for n, p in model.named_parameters()}
    for k, v in model.state_dict().items():
        if k.endswith(BUFFERS):
            assert np.array_equal(v.detach().numpy().astype(state[k].dtype), state[k]), f"the reference moved {k} in eval mode"
    return logits.detach().numpy().copy(), float(loss.detach()), grads, float(min(margins) if margins else 1.0)


def product_grad_error(arch, ncls, state, x, target, grads):
    """The seed screen of oracle/gen_golden_finetune.py for this mode: worst projected relative gradient distance of the product's
    host logic on the torch checker backend (eval-mode model)."""
    from cpu_ops_eval import CpuOpsEval
    from rspnet_amd import ops
    from rspnet_amd.models import get_model_class
    from rspnet_amd.moco.split_wrapper import MultiTaskWrapper
    prev = ops.set_backend(CpuOpsEval())
    try:
        model = MultiTaskWrapper(get_model_class(arch=arch), num_classes=ncls, finetune=True)
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
        model.eval()
        loss = torch.nn.CrossEntropyLoss()(model(torch.from_numpy(x)), torch.from_numpy(target))
        loss.backward()
        return max(P.proj_rel_err(n, p.grad.numpy(), P.projections(n, grads[n])) for n, p in model.named_parameters()
                   if grads[n] is not None and float(np.sqrt((grads[n].astype(np.float64) ** 2).sum())) >= 1e-4)
    finally:
        ops.set_backend(prev)


def fp64_floor(arch, ncls, state, x, target, grads):
    """Worst per-parameter relative L2 distance between the reference's fp32 gradients and its own fp64 evaluation."""
    model64 = R.build_reference_finetune(arch, ncls)
    _, _, g64, _ = run_reference_eval(model64, state, x, target, dtype=torch.float64)
    worst = 0.0
    for n, g in grads.items():
        if g is None:
            continue
        ref = g64[n].astype(np.float64)
        norm = float(np.sqrt((ref ** 2).sum()))
        if norm >= 1e-4:
            worst = max(worst, float(np.sqrt(((g.astype(np.float64) - ref) ** 2).sum())) / norm)
    return worst


def main():
    torch.manual_seed(0)
    only = sys.argv[1:]
    for arch, B, T, HW, ncls, seed0 in CASES:
        if only and arch not in only:
            continue
        model = R.build_reference_finetune(arch, ncls)
        spec = R.state_spec(model)
        gate = SEED_GATE.get(arch, 3e-4)
        screened = True
        tried = []
        for seed in range(seed0, seed0 + 24):
            state = P.fill_state(spec, seed)
            x = P.clips(seed, 0, (B, 3, T, HW, HW))[0]
            target = ((np.arange(B) * 3 + seed) % ncls).astype(np.int64)
            nudges, rep = guard.guard_band(arch, "linear", state, [x],
                                           forward=lambda sd, xx: S.finetune_forward(arch, sd, xx, training=False))
            guard.apply_nudges(state, nudges)
            print(f"{arch} seed {seed}: guard {rep}", flush=True)
            logits, loss, grads, margin = run_reference_eval(model, state, x, target)
            perr = product_grad_error(arch, ncls, state, x, target, grads)
            print(f"{arch} seed {seed}: checker-backend gradient error {perr:.1e}, ReLU / pool margin {margin:.1e}", flush=True)
            tried.append((perr, seed, state, x, target, nudges, logits, loss, grads, margin))
            if perr <= gate and (margin >= 3e-6 or arch == "s3dg"):
                break
        else:
            if arch != "s3dg":
                raise SystemExit(f"{arch}: no well-conditioned seed found")
            # S3D-G: no seed under its screen — ship the best one seen, with its measured floor, and say so
            screened = False
            tried.sort(key=lambda t: t[0])
        perr, seed, state, x, target, nudges, logits, loss, grads, margin = tried[-1] if screened else tried[0]
        # restatement vs reference (eval forward)
        sd = {k: torch.from_numpy(v.copy()) for k, v in state.items()}
        e1 = float((S.finetune_forward(arch, sd, torch.from_numpy(x), training=False) - torch.from_numpy(logits)).abs().max())
        assert e1 <= 1e-5, e1
        floor = fp64_floor(arch, ncls, state, x, target, grads)
        print(f"{arch}: seed {seed}, loss {loss:.5f}, checker error {perr:.1e}, margin {margin:.1e}, fp32-vs-fp64 floor {floor:.2e}, "
              f"screened {screened}", flush=True)
        meta = {"arch": arch, "B": B, "T": T, "HW": HW, "classes": ncls, "seed": seed, "mode": "eval", "floor": floor,
                "checker_err": perr, "margin": margin, "screened": screened}
        out = {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), "target": target, "logits": logits,
               "loss": np.float64(loss)}
        for k, g in grads.items():
            out["gradsum." + k] = np.zeros(0) if g is None else P.summarise(k, g)
            if g is not None:
                out["gradproj." + k] = P.projections(k, g)
        for k, (idx, val) in nudges.items():
            out["nudge.idx." + k] = np.asarray(idx, dtype=np.int32)
            out["nudge.val." + k] = np.asarray(val, dtype=np.float32)
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", f"finetune_frozen_bn_{arch.replace('-', '_')}.npz"), **out)


if __name__ == "__main__":
    main()
