"""CPU: host logic of fine-tuning with frozen BatchNorm (backward through an eval-mode backbone) on the torch checker backend
extended with the eval-mode op (tests/cpu_ops_eval.py), against the eval-mode fixtures of the reference."""
import numpy as np
import pytest
import torch

from cpu_ops import CpuOps
from cpu_ops_eval import CpuOpsEval
from frozen_bn_util import ARCHS, check_case, load
from finetune_util import build_model
from golden_util import fwd_tol
from rspnet_amd import ops


@pytest.fixture()
def cpu_eval_backend():
    prev = ops.set_backend(CpuOpsEval())
    yield
    ops.set_backend(prev)


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())
    yield
    ops.set_backend(prev)


@pytest.mark.parametrize("arch", ARCHS)
def test_eval_mode_forward_backward_matches_fixture(cpu_eval_backend, arch):
    _, model, z, meta = check_case(arch, torch.device("cpu"), fwd_tol(arch, 2e-4))
    if arch == "c3d":
        # a conv bias in front of BatchNorm on running statistics has a real gradient (train mode cancels it)
        for n, p in model.named_parameters():
            if n.startswith("encoder.conv") and n.endswith(".bias"):
                assert float(z["gradsum." + n][0]) >= 1e-4 and float(p.grad.norm()) > 0, n
    if arch == "r2plus1d-vcop":
        # channel-padded units (mid-channel counts that are no multiple of 4): gradients keep the parameters' own shapes
        assert any(p.dim() == 1 and p.shape[0] % 4 for n, p in model.named_parameters() if n.startswith("encoder."))
        assert all(p.grad is None or p.grad.shape == p.shape for p in model.parameters())


def test_backend_without_the_op_keeps_the_error(cpu_backend):
    z, meta, state, x = load("c3d")
    model = build_model("c3d", meta["classes"], state, torch.device("cpu"))
    model.eval()
    loss = torch.nn.CrossEntropyLoss()(model(torch.from_numpy(x)), torch.from_numpy(z["target"]))
    with pytest.raises(RuntimeError) as exc:
        loss.backward()
    assert str(exc.value) == ("backward through an eval-mode backbone (BatchNorm on running statistics) is not implemented: "
                              "freeze the backbone (only_train_fc) or call model.train()")


def test_forward_ndhwc_still_refuses_keep_in_eval_mode(cpu_eval_backend):
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory as PretextFactory
    pre = PretextFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=torch.device("cpu")).module
    x = torch.zeros(1, 4, 16, 16, 4)
    with pytest.raises(ValueError):
        pre.encoder_q.forward_ndhwc(x, keep=True, training=False)


def test_factory_freeze_bn_keys(cpu_eval_backend):
    """freeze_bn: train() keeps the encoder in eval mode, requires_grad untouched; freeze_bn_affine: BatchNorm weight / bias get no
    gradient while conv weights AND conv biases still do; only_train_fc wins over both."""
    from rspnet_amd.models import ModelFactory
    z, meta, state, x = load("c3d")
    cfg = {"model": {"arch": "c3d"}, "dataset": {"num_classes": meta["classes"]}}
    xt, tt = torch.from_numpy(x), torch.from_numpy(z["target"])

    model = ModelFactory({**cfg, "freeze_bn": True})._post_process_model(build_model("c3d", meta["classes"], state, torch.device("cpu")))
    model.train()
    assert not model.encoder.training and model.fc.training and all(p.requires_grad for p in model.parameters())
    buffers = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    logits = model(xt)
    torch.nn.CrossEntropyLoss()(logits, tt).backward()
    assert np.allclose(logits.detach().numpy(), z["logits"], atol=2e-4 * float(abs(z["logits"]).max()))
    assert model.encoder.bn1.weight.grad is not None and model.encoder.conv1.weight.grad is not None
    assert all(torch.equal(model.state_dict()[k], v) for k, v in buffers.items())
    full = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()
    assert not model.encoder.training and not model.fc.training

    model = ModelFactory({**cfg, "freeze_bn": True, "freeze_bn_affine": True})._post_process_model(
        build_model("c3d", meta["classes"], state, torch.device("cpu")))
    model.train()
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen and all(n.startswith("encoder.bn") for n in frozen)
    torch.nn.CrossEntropyLoss()(model(xt), tt).backward()
    assert model.encoder.bn1.weight.grad is None and model.encoder.bn5b.bias.grad is None
    # the conv bias gradient still comes out of the kernel's dbeta sums, and nothing else changed
    for n, p in model.named_parameters():
        if p.requires_grad and p.grad is not None:
            assert torch.equal(p.grad, full[n]), n
    assert float(model.encoder.conv2.bias.grad.norm()) > 0

    model = ModelFactory({**cfg, "freeze_bn": True, "only_train_fc": True})._post_process_model(
        build_model("c3d", meta["classes"], state, torch.device("cpu")))
    model.train()
    assert [n for n, p in model.named_parameters() if p.requires_grad] == ["fc.weight", "fc.bias"]
    torch.nn.CrossEntropyLoss()(model(xt), tt).backward()
    assert model.encoder.conv1.weight.grad is None and model.fc.weight.grad is not None
