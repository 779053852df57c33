"""GPU: fine-tuning with frozen BatchNorm — model.eval(), forward, CrossEntropyLoss, backward through the one-pass eval-mode
BatchNorm backward — against fixtures generated from the reference in eval mode.  Logits / loss at the north-star 1e-3, every
gradient summary at the fixture's gate (three fp32-vs-fp64 floors of the reference, never below 3e-3)."""
import pytest
import torch

from frozen_bn_util import ARCHS, check_case, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("arch", ARCHS)
def test_eval_mode_forward_backward_matches_fixture(arch):
    from frozen_bn_util import gate
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    _, model, z, meta = check_case(arch, DEV, 1e-3)
    if arch == "c3d":
        # conv biases in front of BatchNorm on running statistics: a real gradient (scale * sum dz), inside the gate
        import numpy as np
        from oracle import portable as P
        for n, p in model.named_parameters():
            if n.startswith("encoder.conv") and n.endswith(".bias"):
                g = z["gradsum." + n]
                mine = p.grad.detach().cpu().numpy()
                assert g[0] >= 1e-4 and float(np.abs(mine).max()) > 0, n
                assert P.proj_rel_err(n, mine, z["gradproj." + n]) <= gate(meta), n


def _factory_model(extra):
    from rspnet_amd.models import ModelFactory
    z, meta, state, x = load("c3d")
    cfg = {"model": {"arch": "c3d"}, "dataset": {"num_classes": meta["classes"]}, **extra}
    wrapped = ModelFactory(cfg).build_multitask_wrapper(0)
    wrapped.module.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return wrapped, torch.from_numpy(x).to(DEV), torch.from_numpy(z["target"]).to(DEV)


def test_factory_freeze_bn_trains_and_leaves_the_statistics():
    from rspnet_amd.finetune import train_step
    wrapped, xt, tt = _factory_model({"freeze_bn": True})
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.SGD(wrapped.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    wrapped.train()
    assert not wrapped.module.encoder.training and wrapped.module.fc.training
    buffers = {k: v.detach().clone() for k, v in wrapped.module.state_dict().items() if "running" in k or "num_batches" in k}
    w0 = wrapped.module.encoder.conv3a.weight.detach().clone()
    losses = [float(train_step(wrapped, crit, opt, xt, tt)["loss"]) for _ in range(8)]
    print("\nfreeze_bn losses:", " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0]
    assert not torch.equal(wrapped.module.encoder.conv3a.weight, w0)          # the backbone trained
    for k, v in buffers.items():
        assert torch.equal(wrapped.module.state_dict()[k], v), k


def test_factory_freeze_bn_affine_and_only_train_fc():
    crit = torch.nn.CrossEntropyLoss()
    wrapped, xt, tt = _factory_model({"freeze_bn": True, "freeze_bn_affine": True})
    wrapped.train()
    crit(wrapped(xt), tt).backward()
    m = wrapped.module
    assert m.encoder.bn1.weight.grad is None and m.encoder.bn1.bias.grad is None
    assert m.encoder.conv1.weight.grad is not None and float(m.encoder.conv1.bias.grad.abs().max()) > 0
    # the same conv gradients as with trainable affine parameters: the no-sums form of the kernel writes the same dy
    ref, _, _ = _factory_model({"freeze_bn": True})
    ref.train()
    crit(ref(xt), tt).backward()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, dict(ref.module.named_parameters())[n].grad), n
    wrapped, xt, tt = _factory_model({"freeze_bn": True, "only_train_fc": True})
    wrapped.train()
    crit(wrapped(xt), tt).backward()
    assert wrapped.module.encoder.conv1.weight.grad is None and wrapped.module.fc.weight.grad is not None
