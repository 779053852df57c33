"""CPU: the similarity maps (MoCoDiffLossTwoFc.cam_visualize) and the visualisation driver on the checker backend, against the
fixtures recorded from the reference's own cam_visualize (tools/gen_golden_cam.py)."""
import os
import random

import numpy as np
import pytest
import torch

import cam_util
from cam_util import ARCHS, MAP_NAMES, CamCpuOps, fixture_inputs, load_fixture, rel_err, restated_maps
from model_util import ReplayRNG, make_cfg
from rspnet_amd import ops
from rspnet_amd.moco import Loss, ModelFactory

CPU = torch.device("cpu")


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CamCpuOps())
    yield
    ops.set_backend(prev)


def build_model(arch, meta, state, fc_type="linear"):
    model = ModelFactory(make_cfg(arch, meta["K"], fc_type=fc_type, speeds=(meta["speed"],))).build_moco_diffloss(device=CPU).module
    if state is not None:
        model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return model


def snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("arch", ARCHS)
def test_fixture_holds_against_fp64_restatement(arch):
    """The stored reference maps against the fp64 restatement of the same call, within the stored floor x 1.5 (the rounding of the
    comparison itself); floors below 1e-4 (the generator's conditioning criterion)."""
    z, meta = load_fixture(arch)
    state, im_q, im_k = fixture_inputs(arch, meta)
    want = restated_maps(arch, state, im_q, im_k, z["perms"], meta["speed"]).numpy()
    assert float(z["floor"].max()) <= 1e-4
    for i, name in enumerate(MAP_NAMES):
        err = rel_err(z[name], want[i])
        print(f"{arch} {name}: fixture vs fp64 restatement {err:.2e}, stored floor {float(z['floor'][i]):.2e}")
        assert z[name].shape == want[i].shape and err <= 1.5 * float(z["floor"][i])


@pytest.mark.parametrize("arch", ARCHS)
def test_cam_visualize_matches_reference_fixture(cpu_backend, arch):
    z, meta = load_fixture(arch)
    state, im_q, im_k = fixture_inputs(arch, meta)
    model = build_model(arch, meta, state).eval()
    q, k = torch.from_numpy(im_q), torch.from_numpy(im_k)
    with ReplayRNG(list(z["perms"]), meta["speed"]):
        got = model.cam_visualize(q, k)
    assert len(got) == 4
    for name, g in zip(MAP_NAMES, got):
        err = rel_err(g.numpy(), z[name])
        print(f"{arch} {name}: checker backend vs reference {err:.2e}")
        assert g.dtype == torch.float32 and tuple(g.shape) == z[name].shape and err <= 1e-4
    # NDHWC features of what the call used stay readable, as in the reference (there NCDHW)
    assert model.encoder_q._get_last_feature().shape[:4] == (meta["B"],) + z["Ms_qA"].shape[1:]
    assert model.encoder_k._get_last_feature().shape == model.encoder_q._get_last_feature().shape

    # align_keys=True: the key maps are the reference's with the key rows put back in the caller's order (row j of the shuffled
    # batch is clip perms[2][j]: its pairing partner changes, so both sides are recomputed by the restatement for that pairing)
    with ReplayRNG(list(z["perms"]), meta["speed"]):
        aligned = model.cam_visualize(q, k, align_keys=True)
    want = restated_maps(arch, state, im_q, im_k, z["perms"], meta["speed"], aligned=True).numpy()
    for i, (name, g) in enumerate(zip(MAP_NAMES, aligned)):
        err = rel_err(g.numpy(), want[i])
        print(f"{arch} {name}: aligned, checker backend vs fp64 restatement {err:.2e}")
        assert err <= 1e-4
    # ... and where a shuffled row happens to be paired with itself the two pairings agree
    sh = z["perms"][2]
    for j in np.nonzero(sh == np.arange(len(sh)))[0]:
        for a, g in zip(aligned, got):
            assert rel_err(a[j].numpy(), g[j].numpy()) <= 1e-5


def test_cam_visualize_leaves_state_and_rng_as_the_reference_does(cpu_backend):
    z, meta = load_fixture("c3d")
    state, im_q, im_k = fixture_inputs("c3d", meta)
    model = build_model("c3d", meta, state).eval()
    before = snapshot(model)
    grads_before = [p.grad for p in model.parameters()]
    q, k = torch.from_numpy(im_q), torch.from_numpy(im_k)
    B = meta["B"]
    for align in (False, True):
        torch.manual_seed(11)
        random.seed(11)
        model.cam_visualize(q, k, align_keys=align)
        after_t, after_r = torch.randperm(16), random.random()
        # the reference's consumption (:424, :428, :375 twice): three randperm(B), one choice
        torch.manual_seed(11)
        random.seed(11)
        torch.randperm(B)
        random.choice(model.diff_speed)
        torch.randperm(B)
        torch.randperm(B)
        assert torch.equal(after_t, torch.randperm(16)) and after_r == random.random()
        after = snapshot(model)
        assert list(after) == list(before)
        for key in before:
            assert torch.equal(before[key], after[key]), key
    assert all(p.grad is g for p, g in zip(model.parameters(), grads_before))
    assert not model.training and all(not m.training for m in model.modules())
    assert all(not p.requires_grad for p in model.encoder_k.parameters()) and all(p.requires_grad for p in model.encoder_q.parameters())


def test_cam_visualize_refuses_what_it_does_not_define(cpu_backend):
    meta = {"K": 64, "speed": 2}
    model = build_model("c3d", meta, None)
    x = torch.zeros(2, 3, 32, 32, 32)
    with pytest.raises(NotImplementedError, match=r"model\.eval\(\)"):
        model.train().cam_visualize(x, x)
    for fc_type in ("mlp", "conv", "convbn"):
        other = build_model("c3d", meta, None, fc_type=fc_type).eval()
        with pytest.raises(NotImplementedError, match="fc_type"):
            other.cam_visualize(x, x)
    with pytest.raises(ValueError, match="keep"):
        model.encoder_q.forward_ndhwc(torch.zeros(2, 16, 32, 32, 4), keep=True, training=False)
    # speednet (second head Linear(feat, 1)) is defined
    sp = build_model("c3d", meta, None, fc_type="speednet").eval()
    maps = sp.cam_visualize(x, x, align_keys=True)
    assert all(m.shape == (2, 2, 2, 2) for m in maps)


def train_step(model, meta, im_q, im_k, perms):
    from rspnet_amd.optim import SGD
    model.train()
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False)
    crit = Loss(margin=2.0, A=1.0, M=1.0)
    with ReplayRNG(list(perms), meta["speed"]):
        out, tgt, rl, rt = model(im_q, im_k)
    loss, _, _ = crit(out, tgt, rl, rt)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss.detach().clone(), out[0].detach().clone(), snapshot(model)


def test_training_step_unchanged_after_cam_visualize(cpu_backend):
    """The feature changes no existing behaviour: a training step taken after an eval-mode cam_visualize call is bit-identical to
    one taken without it (host-logic fixture: the golden C3D state and clips, checker backend)."""
    z, meta = load_fixture("c3d")
    state, im_q, im_k = fixture_inputs("c3d", meta)
    q, k = torch.from_numpy(im_q), torch.from_numpy(im_k)
    plain = train_step(build_model("c3d", meta, state), meta, q, k, z["perms"])
    model = build_model("c3d", meta, state).eval()
    for align in (False, True):
        with ReplayRNG(list(z["perms"]), meta["speed"]):
            model.cam_visualize(q, k, align_keys=align)
    after = train_step(model, meta, q, k, z["perms"])
    assert torch.equal(plain[0], after[0]) and torch.equal(plain[1], after[1])
    for key in plain[2]:
        assert torch.equal(plain[2][key], after[2][key]), key


def test_overlay_restatement_definition():
    """The colour map and the max == min rule of the restatement the GPU test holds the kernel to."""
    v = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], dtype=torch.float64)
    assert torch.equal(cam_util.jet(v), torch.tensor([[0, 0, 0.5], [0, 0.5, 1], [0.5, 1, 0.5], [1, 0.5, 0], [0.5, 0, 0]],
                                                     dtype=torch.float64))
    clip = torch.full((1, 3, 2, 8, 8), 0.5)
    flat = cam_util.cam_overlay_ref(torch.full((1, 2, 2, 2), 3.0), clip, None, 1)
    want = torch.round(0.6 * 127.5 + 0.4 * 255 * cam_util.jet(torch.tensor(0.0, dtype=torch.float64))).to(torch.uint8)
    assert flat.shape == (1, 8, 8, 3) and bool((flat == want).all())


def test_driver_writes_the_reference_file_names(cpu_backend, tmp_path):
    from PIL import Image
    from rspnet_amd import visualization as vis
    assert callable(ops.HipOps.cam_maps) and callable(ops.HipOps.cam_overlay)
    B, T, size = 2, 32, 32
    g = torch.Generator().manual_seed(5)
    loader = [((torch.rand(B, 3, T, size, size, generator=g), torch.rand(B, 3, T, size, size, generator=g)), torch.zeros(B))
              for _ in range(2)]
    cfg = os.path.join(cam_util.ROOT, "rspnet_amd", "config", "pretrain", "c3d.json")
    exp = tmp_path / "vis"
    over = '{"batch_size": %d, "moco": {"k": 64}}' % B
    written = vis.main(["-c", cfg, "-e", str(exp), "--steps", "2", "--seed", "1", "-x", over], loader=loader, device="cpu")
    names = sorted(os.listdir(exp))
    assert names == sorted(f"iter-{i}-{p}-0.png" for i in range(2) for p in ("RSP", "AVID"))
    assert sorted(os.path.basename(p) for p in written) == names
    for name in names:
        img = Image.open(exp / name)
        assert img.mode == "RGB" and img.size == (2 * size + 30, size + 40)
        a = np.asarray(img)
        assert a.dtype == np.uint8 and len(np.unique(a.reshape(-1, 3), axis=0)) > 1
    exp2 = tmp_path / "all"
    vis.main(["-c", cfg, "-e", str(exp2), "--steps", "1", "--all-samples", "--frame", "0", "-x", over], loader=loader, device="cpu")
    assert sorted(os.listdir(exp2)) == sorted(f"iter-0-{p}-b{b}-0.png" for b in range(B) for p in ("RSP", "AVID"))
    with pytest.raises(ValueError, match="--frame"):
        vis.main(["-c", cfg, "-e", str(exp2), "--steps", "1", "--frame", str(T), "-x", over], loader=loader, device="cpu")
