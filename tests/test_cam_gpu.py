"""GPU: rsp_cam_maps / rsp_cam_overlay against their fp64 restatements, cam_visualize on the HIP backend against the fixtures
recorded from the reference, and the visualisation driver end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cam_util
from cam_util import ARCHS, MAP_NAMES, cam_maps_ref, cam_overlay_ref, fixture_inputs, load_fixture, rel_err, restated_maps
from model_util import ReplayRNG, make_cfg
from rspnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KERNEL_GATE = 2e-5          # the project's per-kernel gate against an exact restatement (tests/test_kernels_gpu.py)

# (B, T', H', W', C): C3D / R(2+1)D, R3D-18, S3D-G, ResNet-50 at their shipped sizes
SHIPPED = [(32, 2, 7, 7, 512), (32, 1, 4, 4, 512), (16, 2, 7, 7, 1024), (8, 1, 4, 4, 2048)]
# seeded geometry fuzz: B = 1, P = 1, C not a multiple of 64 (nor of 4), dim_M = 1 (speednet); (B, T', H', W', C, dim_A, dim_M, pitch)
FUZZ = [(1, 1, 1, 1, 24, 16, 16, 0), (1, 2, 3, 3, 83, 128, 1, 0), (3, 1, 1, 1, 130, 32, 32, 0), (5, 2, 2, 3, 130, 128, 128, 144),
        (4, 1, 5, 2, 83, 7, 7, 96), (7, 3, 1, 2, 512, 128, 128, 640), (2, 1, 1, 9, 24, 3, 5, 24), (9, 2, 7, 7, 64, 128, 128, 0)]


# Where maps_case / check_maps / the overlay body place their operands on the device.  tests/test_guarded_downstream_gpu.py runs them
# with dev() pointed at guarded allocations (tests/guarded.py).
def dev(t):
    return t.to(DEV)


def maps_case(seed, B, Tp, Hp, Wp, C, dim_A=128, dim_M=128, pitch=0, identity=True):
    """Features relu(N(0, 1)), weights N(0, 1 / C); pitch > C: the features are channel slices of a wider tensor."""
    g = torch.Generator().manual_seed(seed)
    feats = []
    for _ in range(2):
        f = torch.relu(torch.randn(B, Tp, Hp, Wp, C, generator=g))
        if pitch:
            wide = torch.full((B, Tp, Hp, Wp, pitch), float("nan"))
            wide[..., :C] = f
            feats.append(dev(wide)[..., :C])
        else:
            feats.append(dev(f))
    ws = [torch.randn(d, C, generator=g) / C ** 0.5 for d in (dim_A, dim_M, dim_A, dim_M)]
    k_row = torch.arange(B) if identity else torch.randperm(B, generator=g)
    return feats, ws, k_row.to(torch.int32)


def check_maps(seed, B, Tp, Hp, Wp, C, dim_A=128, dim_M=128, pitch=0, identity=True):
    (fq, fk), ws, k_row = maps_case(seed, B, Tp, Hp, Wp, C, dim_A, dim_M, pitch, identity)
    be = ops.backend()
    kd, wd = dev(k_row), [dev(w) for w in ws]
    out = be.cam_maps(fq, fk, kd, *wd)
    again = be.cam_maps(fq, fk, kd, *wd)
    assert out.shape == (4, B, Tp, Hp, Wp) and out.dtype == torch.float32
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))          # run-to-run bit-identical
    ncdhw = lambda x: x.cpu().permute(0, 4, 1, 2, 3)
    want = cam_maps_ref(ncdhw(fq), ncdhw(fk), k_row, *ws)
    errs = [rel_err(out[i].cpu().numpy(), want[i].numpy()) for i in range(4)]
    print(f"cam_maps B={B} P={Tp * Hp * Wp} C={C} dims=({dim_A},{dim_M}) pitch={pitch or C} identity={identity}: "
          + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= KERNEL_GATE, errs


@pytest.mark.parametrize("shape", SHIPPED)
def test_cam_maps_shipped_shapes(shape):
    check_maps(1, *shape)
    check_maps(2, *shape, identity=False)


@pytest.mark.parametrize("case", FUZZ)
def test_cam_maps_geometry_fuzz(case):
    B, Tp, Hp, Wp, C, dA, dM, pitch = case
    check_maps(3 + C, B, Tp, Hp, Wp, C, dA, dM, pitch, identity=False)
    check_maps(4 + C, B, Tp, Hp, Wp, C, dA, dM, pitch, identity=True)


def test_cam_maps_rejects_bad_arguments():
    from rspnet_amd import _lib
    (fq, fk), ws, k_row = maps_case(1, 2, 1, 2, 2, 64)
    be = ops.backend()
    with pytest.raises(_lib.RspError):
        be.cam_maps(fq, fk[:1], k_row.to(DEV), *[w.to(DEV) for w in ws])
    with pytest.raises(_lib.RspError):
        be.cam_maps(fq, fk, k_row.to(DEV).long(), *[w.to(DEV) for w in ws])
    with pytest.raises(_lib.RspError):
        be.cam_maps(fq.cpu(), fk, k_row.to(DEV), *[w.to(DEV) for w in ws])
    # a pairing index outside [0, B) poisons that sample's maps and nothing else (no out-of-bounds read)
    bad = torch.tensor([1, 7], dtype=torch.int32, device=DEV)
    out = be.cam_maps(fq, fk, bad, *[w.to(DEV) for w in ws])
    assert bool(torch.isnan(out[:, 1]).all()) and bool(torch.isfinite(out[:, 0]).all())


def build_model(arch, meta, state):
    from rspnet_amd.moco import ModelFactory
    model = ModelFactory(make_cfg(arch, meta["K"], speeds=(meta["speed"],))).build_moco_diffloss(device=DEV).module
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return model


@pytest.mark.parametrize("arch", ARCHS)
def test_cam_visualize_matches_reference_fixture(arch):
    """Gate per map, relative to the map's max-abs: max(3 x the fixture's conditioning floor, 1e-4) — three floors is the rule for
    gates that sit on a conditioning measurement (tests/golden_util.py); 1e-4 is the gate of eval-mode get_feature against
    reference fixtures (tests/test_retrieval_gpu.py), of which the maps are a bilinear function.  Measured on the MI355X (worst map):
    C3D 3.1e-6, R3D-18 2.0e-6, R(2+1)D 2.5e-6, S3D-G 4.0e-6; aligned keys 3.0e-6 / 1.5e-6 / 2.4e-6 / 3.2e-6."""
    assert ops.backend().name == "hip"
    z, meta = load_fixture(arch)
    state, im_q, im_k = fixture_inputs(arch, meta)
    model = build_model(arch, meta, state).eval()
    q, k = torch.from_numpy(im_q).to(DEV), torch.from_numpy(im_k).to(DEV)
    with ReplayRNG(list(z["perms"]), meta["speed"]):
        got = model.cam_visualize(q, k)
    for i, (name, g) in enumerate(zip(MAP_NAMES, got)):
        err, gate = rel_err(g.cpu().numpy(), z[name]), max(3 * float(z["floor"][i]), 1e-4)
        print(f"{arch} {name}: HIP vs reference fixture {err:.2e} (gate {gate:.1e})")
        assert g.device == q.device and g.dtype == torch.float32 and tuple(g.shape) == z[name].shape and err <= gate
    with ReplayRNG(list(z["perms"]), meta["speed"]):
        aligned = model.cam_visualize(q, k, align_keys=True)
    want = restated_maps(arch, state, im_q, im_k, z["perms"], meta["speed"], aligned=True).numpy()
    for i, (name, g) in enumerate(zip(MAP_NAMES, aligned)):
        err, gate = rel_err(g.cpu().numpy(), want[i]), max(3 * float(z["floor"][i]), 1e-4)
        print(f"{arch} {name}: HIP aligned vs fp64 restatement {err:.2e} (gate {gate:.1e})")
        assert err <= gate


def _train_step(model, meta, q, k, perms):
    from rspnet_amd.moco import Loss
    from rspnet_amd.optim import SGD
    model.train()
    opt = SGD(model.parameters(), lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False)
    with ReplayRNG(list(perms), meta["speed"]):
        out, tgt, rl, rt = model(q, k)
    loss, _, _ = Loss(margin=2.0, A=1.0, M=1.0)(out, tgt, rl, rt)
    opt.zero_grad()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return loss.detach().clone(), out[0].detach().clone(), {n: v.detach().clone() for n, v in model.state_dict().items()}


def test_state_untouched_and_following_step_unchanged():
    z, meta = load_fixture("c3d")
    state, im_q, im_k = fixture_inputs("c3d", meta)
    q, k = torch.from_numpy(im_q).to(DEV), torch.from_numpy(im_k).to(DEV)
    plain = _train_step(build_model("c3d", meta, state), meta, q, k, z["perms"])
    model = build_model("c3d", meta, state).eval()
    before = {n: v.detach().clone() for n, v in model.state_dict().items()}
    for align in (False, True):
        with ReplayRNG(list(z["perms"]), meta["speed"]):
            model.cam_visualize(q, k, align_keys=align)
    after = model.state_dict()
    assert list(after) == list(before)
    for n in before:
        assert torch.equal(before[n], after[n]), n
    assert all(p.grad is None for p in model.parameters())
    step = _train_step(model, meta, q, k, z["perms"])
    assert torch.equal(plain[0], step[0]) and torch.equal(plain[1], step[1])
    for n in plain[2]:
        assert torch.equal(plain[2][n], step[2][n]), n


@pytest.mark.parametrize("size", [112, 224])
@pytest.mark.parametrize("Tp", [1, 2])
def test_cam_overlay_matches_restatement(size, Tp):
    """Every channel of every pixel within 1 (of 255); N(0, 1) maps (a wide min-max range), one constant map (max == min: v = 0)."""
    g = torch.Generator().manual_seed(size + Tp)
    B, T, t = 3, 4, 2
    maps = torch.randn(4 * B, Tp, 7, 5 if Tp == 2 else 7, generator=g)
    maps[5] = 0.25
    clip_a, clip_b = torch.rand(B, 3, T, size, size, generator=g), torch.rand(B, 3, T, size, size, generator=g)
    be = ops.backend()
    md, ad, bd = dev(maps), dev(clip_a), dev(clip_b)
    out = be.cam_overlay(md, ad, bd, t)
    assert out.shape == (4 * B, size, size, 3) and out.dtype == torch.uint8
    assert torch.equal(out, be.cam_overlay(md, ad, bd, t))
    want = cam_overlay_ref(maps, clip_a, clip_b, t)
    diff = (out.cpu().to(torch.int16) - want.to(torch.int16)).abs()
    print(f"cam_overlay size={size} T'={Tp}: max diff {int(diff.max())}, pixels off by one {int((diff > 0).sum())} of {diff.numel()}")
    assert int(diff.max()) <= 1
    # one clip for all panels
    single = be.cam_overlay(md[:B], ad, None, 0)
    assert int((single.cpu().to(torch.int16) - cam_overlay_ref(maps[:B], clip_a, None, 0).to(torch.int16)).abs().max()) <= 1


def test_driver_end_to_end(tmp_path):
    """python -m rspnet_amd.visualization at C3D 112 x 112, B = 4, two steps, in a child process under a time limit."""
    from PIL import Image
    exp = tmp_path / "vis"
    cfg = os.path.join(cam_util.ROOT, "rspnet_amd", "config", "pretrain", "c3d.json")
    r = subprocess.run([sys.executable, "-m", "rspnet_amd.visualization", "-c", cfg, "-e", str(exp), "--steps", "2", "--seed", "3",
                        "-x", '{"batch_size": 4}'], cwd=cam_util.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(exp))
    assert names == sorted(f"iter-{i}-{p}-0.png" for i in range(2) for p in ("RSP", "AVID"))
    for name in names:
        img = Image.open(exp / name)
        a = np.asarray(img)
        assert img.mode == "RGB" and a.dtype == np.uint8 and a.shape == (112 + 40, 2 * 112 + 30, 3)
        panels = np.concatenate([a[10:122, 10:122], a[10:122, 132:244]])
        assert len(np.unique(panels.reshape(-1, 3), axis=0)) > 16          # not all one colour
