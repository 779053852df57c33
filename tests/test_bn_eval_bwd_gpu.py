"""GPU: the one-pass eval-mode BatchNorm backward (rsp_bn_eval_act_pool_bwd through HipOps.bn_eval_act_pool_bwd) against torch
autograd in fp32 on the same device, over  pool(relu(y * scale + shift + residual))  with the affine parameters as leaves
(scale = gamma * invstd, shift = beta - mean' * scale).  Per-kernel tolerance of the suite: 2e-5 relative to each output's max.

Inputs are continuous random values, so pool ties do not occur; the few elements whose pre-activation torch computes within 1e-4 of
zero are moved off it (a ReLU decision inside the rounding band is not what these tests are about)."""
import random

import pytest
import torch
import torch.nn.functional as F

from rspnet_amd.ops import PoolGeom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL = 2e-5


# Where the test bodies place their operands on the device.  tests/test_guarded_memory_gpu.py runs the same bodies with these two
# pointed at guarded allocations (tests/guarded.py): dev() for inputs, dev_empty() for what a kernel writes.
def dev(t):
    return t.to(DEV)


def dev_empty(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def hip():
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    return ops.backend()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def close(a, b, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item()
    ref = max(b.abs().max().item(), 1e-6)
    print(f"{what}: rel err {err / ref:.2e}")
    assert err <= TOL * ref, f"{what}: max err {err:.3e} vs ref max {ref:.3e} (rel {err / ref:.3e} > {TOL})"


def make_case(N, D, H, W, C, k, relu, use_res, Cv=None, wide=0):
    """Device inputs.  wide > 0: y, dout (and the dy output) are channel slices [wide, wide + C) of tensors 2 * wide + C wide."""
    Cv = C if Cv is None else Cv
    pg = PoolGeom(N, D, H, W, C, k, k, (0, 0, 0))
    gamma, beta = dev(rnd(Cv, seed=3) + 1.5), dev(rnd(Cv, seed=4) * 0.5)
    meanp, invstd = dev(rnd(C, seed=6) * 0.3), dev(rnd(C, seed=7) * 0.4 + 1.0)
    pad = dev_empty(C - Cv).zero_()
    scale = torch.cat([gamma, pad]) * invstd
    shift = torch.cat([beta, pad]) - meanp * scale
    y = dev(rnd(N, D, H, W, C, seed=1) * 2)
    res = dev(rnd(N, D, H, W, C, seed=2)) if use_res else None
    z = y * scale + shift + (res if use_res else 0)
    near = (z.abs() < 1e-4) & (scale != 0)
    y = dev(torch.where(near, y + torch.where(z >= 0, 3e-4, -3e-4) / torch.where(scale != 0, scale, torch.ones_like(scale)), y))
    do, ho, wo = pg.out_dims
    dout = dev(rnd(N, do, ho, wo, C, seed=5))
    if wide:
        yw = dev_empty((N, D, H, W, C + 2 * wide)).fill_(float("nan"))
        yw[..., wide:wide + C] = y
        y = yw[..., wide:wide + C]
        dw = dev_empty((N, do, ho, wo, C + 2 * wide)).fill_(float("nan"))
        dw[..., wide:wide + C] = dout
        dout = dw[..., wide:wide + C]
    mi = dev(torch.stack([meanp, invstd]).contiguous())
    ss = dev(torch.stack([scale, shift]).contiguous())
    return pg, y, res, dout, gamma, beta, meanp, invstd, mi, ss, Cv


def reference(pg, y, res, dout, gamma, beta, meanp, invstd, relu, Cv):
    C = y.shape[-1]
    g = gamma.clone().requires_grad_(True)
    b = beta.clone().requires_grad_(True)
    yy = y.detach().clone().contiguous().requires_grad_(True)
    rr = res.detach().clone().requires_grad_(True) if res is not None else None
    pad = torch.zeros(C - Cv, device=y.device)
    scale = torch.cat([g, pad]) * invstd
    shift = torch.cat([b, pad]) - meanp * scale
    z = yy * scale + shift
    if rr is not None:
        z = z + rr
    a = F.relu(z) if relu else z
    if pg.k != (1, 1, 1):
        a = F.max_pool3d(a.permute(0, 4, 1, 2, 3), pg.k, pg.s).permute(0, 2, 3, 4, 1)
    leaves = [yy, g, b] + ([rr] if rr is not None else [])
    grads = torch.autograd.grad(a, leaves, dout.contiguous())
    return grads[0], grads[1], grads[2], (grads[3] if rr is not None else None)


def run_op(hip, pg, y, res, dout, mi, ss, relu, Cv, sums=True, wide=0):
    dg = dev_empty((Cv,)).fill_(float("nan")) if sums else None
    db = dev_empty((Cv,)).fill_(float("nan")) if sums else None
    dy_out = None
    if wide:
        dyw = dev_empty(tuple(y.shape[:4]) + (y.shape[4] + 2 * wide,)).fill_(7.0)
        dy_out = dyw[..., wide:wide + y.shape[4]]
    dy, dres = hip.bn_eval_act_pool_bwd(pg, y, res, dout, mi, ss, relu, res is not None, dg, db, dy_out=dy_out)
    torch.cuda.synchronize()
    if wide:      # nothing outside the slice was written
        assert bool((dyw[..., :wide] == 7.0).all()) and bool((dyw[..., wide + y.shape[4]:] == 7.0).all())
    return dy, dres, dg, db


def check(hip, N, D, H, W, C, k, relu, use_res, Cv=None, wide=0):
    pg, y, res, dout, gamma, beta, meanp, invstd, mi, ss, Cv = make_case(N, D, H, W, C, k, relu, use_res, Cv, wide)
    dy_ref, dg_ref, db_ref, dres_ref = reference(pg, y, res, dout, gamma, beta, meanp, invstd, relu, Cv)
    dy, dres, dg, db = run_op(hip, pg, y, res, dout, mi, ss, relu, Cv, True, wide)
    close(dy, dy_ref, "dy")
    close(dg, dg_ref, "dgamma")
    close(db, db_ref, "dbeta")
    if use_res:
        close(dres, dres_ref, "dres")
    if Cv < C:
        assert bool((dy[..., Cv:] == 0).all()), "padding channels of dy must be exactly zero"
    # frozen affine parameters: no sums, the same dy / dres bit for bit
    dy0, dres0, _, _ = run_op(hip, pg, y, res, dout, mi, ss, relu, Cv, False, wide)
    assert torch.equal(dy0, dy)
    if use_res:
        assert torch.equal(dres0, dres)
    # run to run: bit-identical (fixed-order partial sums, no atomics)
    dy2, dres2, dg2, db2 = run_op(hip, pg, y, res, dout, mi, ss, relu, Cv, True, wide)
    assert torch.equal(dy2, dy) and torch.equal(dg2, dg) and torch.equal(db2, db)
    if use_res:
        assert torch.equal(dres2, dres)


CASES = [
    # N, D, H, W, C, k, relu, residual, c_valid, wide
    (2, 3, 7, 7, 64, (1, 1, 1), True, False, None, 0),        # unit window
    (2, 3, 7, 7, 64, (1, 1, 1), False, False, None, 0),       # BatchNorm only (shortcut branch)
    (2, 3, 5, 5, 64, (1, 1, 1), True, True, None, 0),         # residual add before the ReLU
    (2, 3, 5, 5, 64, (1, 1, 1), False, True, None, 0),
    (2, 4, 8, 8, 64, (1, 2, 2), True, False, None, 0),        # C3D pool1
    (2, 4, 8, 8, 128, (2, 2, 2), True, False, None, 0),       # C3D pool2-4
    (2, 4, 8, 8, 32, (2, 2, 2), False, True, None, 0),
    (2, 5, 7, 7, 64, (2, 2, 2), True, False, None, 0),        # windows do not tile the input: the tail gets dy = 0
    (2, 4, 7, 9, 16, (1, 2, 2), True, True, None, 0),
    (1, 6, 6, 6, 8, (3, 3, 3), True, False, None, 0),         # 27-position windows
    (2, 8, 6, 6, 8, (4, 2, 2), True, False, None, 0),         # 16-position windows
    (2, 3, 5, 5, 4, (1, 1, 1), True, False, None, 0),         # C = 4
    (2, 3, 5, 5, 832, (1, 1, 1), True, False, None, 0),       # C = 832 (S3D-G mixed_5b)
    (1, 2, 4, 4, 1152, (1, 1, 1), True, False, None, 0),      # > 1024 channels: two channel chunks
    (2, 3, 5, 5, 83, (1, 1, 1), True, False, None, 0),        # odd channel count: scalar path
    (2, 3, 6, 6, 84, (1, 1, 1), True, False, 83, 0),          # channel-padded unit (R(2+1)D): c_valid < C
    (2, 4, 6, 6, 232, (1, 2, 2), True, False, 230, 0),
    (2, 4, 7, 7, 64, (1, 1, 1), True, False, None, 32),       # channel slices of wider tensors (into nodes, S3D-G) + dy_out
    (2, 4, 8, 8, 48, (1, 2, 2), True, False, None, 16),
    (2, 8, 72, 64, 64, (1, 1, 1), True, False, None, 0),      # 73 728 positions: hundreds of workgroups' partials
    (2, 8, 72, 64, 64, (2, 2, 2), True, False, None, 0),
    (1, 3, 33, 31, 64, (1, 1, 1), True, True, None, 0),       # a ragged last trip of the streaming body
]


def _fuzz(n=24, seed=20261017):
    """Seeded random geometries: ragged sizes, disjoint windows that may not tile the input, odd and padded channel counts."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = tuple(rng.choice((1, 1, 2, 3)) for _ in range(3))
        D, H, W = (rng.randint(kk, 9) for kk in k)
        C = rng.choice((4, 8, 32, 64, 83, 96, 260, 480, 832))
        Cv = C - rng.randint(1, 3) if (C % 4 == 0 and C > 4 and rng.random() < 0.25) else None
        wide = rng.choice((0, 0, 16)) if C % 4 == 0 else 0
        out.append((rng.randint(1, 3), D, H, W, C, k, rng.random() < 0.8, rng.random() < 0.4, Cv, wide))
    return out


@pytest.mark.parametrize("case", CASES + _fuzz(), ids=lambda c: "x".join(map(str, c[:5])) + f"k{c[5]}r{int(c[6])}{int(c[7])}v{c[8]}w{c[9]}")
def test_bn_eval_act_pool_bwd_matches_autograd(hip, case):
    check(hip, *case)


def test_sums_only_for_one_parameter(hip):
    """dbeta alone (a conv-bias gradient with frozen affine parameters) or dgamma alone: the same sums as with both."""
    pg, y, res, dout, gamma, beta, meanp, invstd, mi, ss, Cv = make_case(2, 4, 8, 8, 64, (1, 2, 2), True, False)
    _, _, dg, db = run_op(hip, pg, y, None, dout, mi, ss, True, Cv)
    db1 = dev_empty(Cv)
    hip.bn_eval_act_pool_bwd(pg, y, None, dout, mi, ss, True, False, None, db1)
    dg1 = dev_empty(Cv)
    hip.bn_eval_act_pool_bwd(pg, y, None, dout, mi, ss, True, False, dg1, None)
    assert torch.equal(db1, db) and torch.equal(dg1, dg)


def test_captured_after_an_eager_call(hip):
    """The entry point only enqueues kernels on the given stream: a HIP graph of it replays to the same bits."""
    pg, y, res, dout, gamma, beta, meanp, invstd, mi, ss, Cv = make_case(2, 4, 8, 8, 64, (2, 2, 2), True, False)
    dy, _, dg, db = run_op(hip, pg, y, None, dout, mi, ss, True, Cv)
    dy_g, dg_g, db_g = torch.empty_like(dy), torch.empty_like(dg), torch.empty_like(db)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            hip.bn_eval_act_pool_bwd(pg, y, None, dout, mi, ss, True, False, dg_g, db_g, dy_out=dy_g)
    torch.cuda.current_stream().wait_stream(s)
    for t in (dy_g, dg_g, db_g):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dy_g, dy) and torch.equal(dg_g, dg) and torch.equal(db_g, db)
