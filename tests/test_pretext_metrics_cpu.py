"""CPU: the torch-ops side of the pretext meters (rspnet_amd.pretrain.pretext_accuracy + PretextMeters.update, what
rsp_pretext_metrics is compared against on the GPU) next to the reference's own framework.metrics.classification.accuracy and
framework.meters.AverageMeter, imported live, and the meter wording against AverageMeter.__str__."""
import os
import sys

import numpy as np
import pytest
import torch

REFERENCE = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "framework")),
                                     reason="/root/reference not present (GPU box)")
BS = (1, 3, 32)
K1S = (5, 63, 64, 65, 257)
NAMES = ("Loss", "Loss_A", "Acc@1_A", "Acc@5_A", "Acc@1_A_n", "Acc@5_A_n", "Loss_M", "Acc@1_M")
FMTS = (":f", ":f", ":6.2f", ":6.2f", ":6.2f", ":6.2f", ":f", ":6.2f")


def reference_modules():
    """framework.metrics.classification and framework.meters.average loaded by file: the package __init__ files pull in more of the
    reference than the two functions under comparison need."""
    import importlib.util
    mods = []
    for name, rel in (("_ref_classification", "framework/metrics/classification.py"), ("_ref_average", "framework/meters/average.py")):
        if name not in sys.modules:
            spec = importlib.util.spec_from_file_location(name, os.path.join(REFERENCE, rel))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            sys.modules[name] = mod
        mods.append(sys.modules[name])
    return mods


def draw(B, K1, seed):
    g = torch.Generator().manual_seed(seed)
    l1, l2 = torch.randn(B, K1, generator=g), torch.randn(B, K1, generator=g)
    lp, ln = torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)
    losses = torch.rand(3, generator=g) * 10
    for m in (l1, l2):      # tie-free: torch.topk leaves the order of tied entries open
        assert not bool((m[:, 1:] == m[:, :1]).any())
    assert not bool((lp == ln).any())
    return l1, l2, lp, ln, losses


@needs_reference
@pytest.mark.parametrize("K1", K1S)
@pytest.mark.parametrize("B", BS)
def test_accuracy_and_meters_equal_the_reference_live(B, K1):
    from rspnet_amd.pretrain import PretextMeters, pretext_accuracy
    cls, avg = reference_modules()
    ref = [avg.AverageMeter(n, fmt=f) for n, f in zip(NAMES, FMTS)]
    meters = PretextMeters("cpu")
    target = torch.zeros(B, dtype=torch.long)
    for call in range(3):
        l1, l2, lp, ln, losses = draw(B, K1, 100 * call + 7 * B + K1)
        acc = pretext_accuracy((l1, l2), (lp, ln))
        a1, a5 = cls.accuracy(l1, target, topk=(1, 5))
        n1, n5 = cls.accuracy(l2, target, topk=(1, 5))
        m1, = cls.accuracy(torch.cat((lp, ln), dim=1), target, topk=(1,))
        want = [losses[0], losses[1], a1, a5, n1, n5, losses[2], m1]
        assert torch.equal(acc, torch.stack([a1, a5, n1, n5, m1]))
        meters.update([losses[0], losses[1], acc[0], acc[1], acc[2], acc[3], losses[2], acc[4]], B)
        for m, v in zip(ref, want):
            m.update(v, B)
        assert torch.equal(meters.val, torch.stack([m.val for m in ref]))
        assert torch.equal(meters.sum, torch.stack([m.sum for m in ref]))
        assert torch.equal(meters.count, torch.stack([m.count for m in ref]))
    stats = meters.read()
    for i, k in enumerate(PretextMeters.KEYS):
        assert stats[k]["avg"] == float(ref[i].avg) and stats[k]["count"] == 3 * B
    assert meters.pieces(stats) == [str(m) for m in ref]
    assert str(meters) == "\t".join(str(m) for m in ref)


def test_names_formats_and_wording():
    from rspnet_amd.pretrain import PretextMeters
    assert PretextMeters.NAMES == NAMES and PretextMeters.FMTS == FMTS
    assert PretextMeters.KEYS == ("loss", "loss_A", "acc1_A", "acc5_A", "acc1_A_n", "acc5_A_n", "loss_M", "acc1_M")
    m = PretextMeters("cpu")
    m.update([torch.tensor(v) for v in (1.5, 0.25, 100.0, 50.0, 3.125, 0.0, 2.0, 75.0)], 4)
    m.update([torch.tensor(v) for v in (0.5, 0.75, 0.0, 50.0, 3.125, 100.0, 4.0, 25.0)], 4)
    # '{name} {val<fmt>} ({avg<fmt>})', framework/meters/average.py:32-38
    assert m.pieces() == ["Loss 0.500000 (1.000000)", "Loss_A 0.750000 (0.500000)", "Acc@1_A   0.00 ( 50.00)", "Acc@5_A  50.00 ( 50.00)",
                          "Acc@1_A_n   3.12 (  3.12)", "Acc@5_A_n 100.00 ( 50.00)", "Loss_M 4.000000 (3.000000)",
                          "Acc@1_M  25.00 ( 50.00)"]
    m.reset()
    assert m.read()["loss"]["count"] == 0 and np.isnan(m.read()["loss"]["avg"])


def test_tie_and_nan_rules_of_the_restatement():
    from rspnet_amd.pretrain import pretext_accuracy
    x = torch.tensor([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],                       # every column ties with the positive: rank 0
                      [0.0, 1.0, 2.0, 3.0, 4.0, 0.0, -1.0],                      # rank 4: top-5, not top-1
                      [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, float("nan")],              # rank 5, the NaN column does not count
                      [float("nan"), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])             # NaN positive: a miss
    lp = torch.tensor([[1.0], [2.0], [float("nan")], [0.0]])
    ln = torch.tensor([[1.0], [3.0], [0.0], [float("nan")]])
    acc = pretext_accuracy((x, x.flip(0)), (lp, ln))
    assert acc.tolist() == [25.0, 50.0, 25.0, 50.0, 25.0]
