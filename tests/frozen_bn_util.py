"""Shared by the frozen-BatchNorm fine-tune tests: load a tests/golden/finetune_frozen_bn_<arch>.npz case (the reference's
MultiTaskWrapper(finetune=True) in EVAL mode: forward, CrossEntropyLoss, backward — tools/gen_golden_frozen_bn.py), run the
product's wrapper on a device / op backend, compare."""
import json
import os

import numpy as np
import torch

from finetune_util import GOLDEN, build_model
from golden_util import rel_err, summary_err
from oracle import portable as P

ARCHS = ["c3d", "resnet18", "r2plus1d-vcop", "s3dg"]
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def load(arch):
    tag = arch.replace("-", "_")
    z = np.load(os.path.join(GOLDEN, f"finetune_frozen_bn_{tag}.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    with open(os.path.join(GOLDEN, f"finetune_spec_{tag}.json")) as f:      # the train-mode fixture's spec: same model
        spec = {k: (tuple(s), d) for k, (s, d) in json.load(f).items()}
    state = P.fill_state(spec, meta["seed"])
    from oracle.gen_golden import nudges_from_npz
    for key, (idx, val) in nudges_from_npz(z).items():      # the fixture's guard band (computed on the eval forward)
        state[key][np.asarray(idx, dtype=np.int64)] = np.asarray(val, dtype=np.float32)
    x = P.clips(meta["seed"], 0, (meta["B"], 3, meta["T"], meta["HW"], meta["HW"]))[0]
    return z, meta, state, x


def gate(meta):
    """The project's convention: three floors, never below 3e-3.  The floor is the reference's own fp32-vs-fp64 gradient
    distance on this case (measured by the generator, stored in the fixture)."""
    return max(3e-3, 3.0 * float(meta["floor"]))


def check_case(arch, device, fwd_tol):
    """model.eval() -> forward -> CrossEntropyLoss -> backward against the fixture.  Returns (worst gradient error, model)."""
    z, meta, state, x = load(arch)
    model = build_model(arch, meta["classes"], state, device)
    before = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(BUFFERS)}
    model.eval()
    logits = model(torch.from_numpy(x).to(device))
    loss = torch.nn.CrossEntropyLoss()(logits, torch.from_numpy(z["target"]).to(device))
    loss.backward()
    e_logits = rel_err(logits.detach().cpu().numpy(), z["logits"])
    e_loss = abs(float(loss.detach()) - float(z["loss"])) / max(1.0, abs(float(z["loss"])))
    print(f"\n{arch}: logits {e_logits:.2e}, loss {e_loss:.2e} (gate {fwd_tol:.0e})")
    assert e_logits <= fwd_tol and e_loss <= fwd_tol
    worst, worst_name = 0.0, None
    for n, p in model.named_parameters():
        g = z["gradsum." + n]
        if g.size == 0:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        mine = p.grad.detach().cpu().numpy()
        if "gradproj." + n in z.files and g[0] >= 1e-4:
            l2 = float(np.sqrt((mine.astype(np.float64) ** 2).sum()))
            err = max(P.proj_rel_err(n, mine, z["gradproj." + n]), abs(l2 - g[0]) / g[0])
        else:
            err = summary_err(n, mine, g)
        if err > worst:
            worst, worst_name = err, n
    print(f"{arch}: worst gradient summary error {worst:.2e} ({worst_name}), gate {gate(meta):.2e} (floor {meta['floor']:.2e})")
    assert worst <= gate(meta), (worst, worst_name)
    # frozen BatchNorm: buffers and counters are the loaded ones, bit for bit
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    return worst, model, z, meta
