"""GPU: pooled-size BatchNorm-backward reduce (ops.bn_act_pool_sel_fwd + bn_act_pool_bwd(..., y_sel=...)).

The forward of a pooled unit that a backward follows also keeps y_sel: the raw convolution output at the position of each window
the arg-max rule selects (first maximum in scan order, as max_pool3d).  The backward's reduce pass then reads dout and y_sel — a
pooled-size tensor — instead of dout and all of y.  Checked here:
  * `out` of the new forward is bn_act_pool_fwd's, bit for bit;
  * y_sel is y gathered at the arg-max that maxpool_fwd (the rule bn_act_maxpool_fwd writes too) reports on the activated tensor;
  * dy, dgamma and dbeta of the backward with y_sel match the existing backward within the per-op replay tolerance, 2e-5 relative
     — and, since the new reduce walks the same positions with the same threads in the same order, bit for bit
    (dy depends on the finalized means of dz and dz * xhat, so its equality covers them).
Cases: pools (1,2,2) and (2,2,2), 64 and 128 channels, position counts that do not fill the last block of a launch, gamma of both
signs, ties inside windows (y on a coarse grid), windows that are negative throughout (every position is a zero after ReLU: the
first one holds the window), with and without ReLU.  Operands in guarded memory (tests/guarded.py)."""
import pytest
import torch

import test_kernels_gpu as K
from guarded import Guarded
from rspnet_amd.ops import PoolGeom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# (N, D, H, W, C, pool, relu)
CASES = [
    (2, 4, 6, 10, 64, (1, 2, 2), True),       # 120 windows: 7.5 position groups of 16
    (2, 4, 6, 10, 128, (2, 2, 2), True),      # 60 windows, 8 positions each
    (1, 2, 14, 18, 64, (2, 2, 2), True),      # 63 windows
    (3, 3, 10, 6, 128, (1, 2, 2), False),     # no ReLU: negative maxima pass their gradient
    (2, 5, 7, 9, 64, (2, 2, 2), True),        # windows that do not tile the input: the tails belong to no window
    (2, 8, 36, 44, 64, (1, 2, 2), True),      # 6336 windows over 50 blocks: one trip of four per thread, then 3 or 4 single ones
]


@pytest.fixture(scope="module")
def hip():
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    return ops.backend()


def _unit(N, D, H, W, C, k, seed=1):
    """y on a grid of 0.25 (ties inside most windows), every fifth window along W negative throughout; gamma of both signs."""
    y = torch.round(K.rnd(N, D, H, W, C, seed=seed) * 8) / 4
    neg = torch.zeros(W, dtype=torch.bool)
    for w0 in range(0, W - 1, 2 * 5):
        neg[w0:w0 + 2] = True
    gamma, beta = K.rnd(C, seed=seed + 2) + 1.5, K.rnd(C, seed=seed + 3) * 0.5
    gamma[1::3] = -gamma[1::3]
    rows = N * D * H * W
    yy = y.reshape(rows, C).double()
    part = torch.stack([yy.sum(0), (yy * yy).sum(0)], 1).float().unsqueeze(0)
    mi, ss = K.CPU.bn_finalize(part, rows, None, gamma, beta, 1e-5, 0.1, None, None)
    # "negative throughout": far on the side of the mean where scale * y + shift < 0, whatever the scale's sign
    far = torch.where(ss[0] > 0, mi[0] - 6.0, mi[0] + 6.0)
    y[:, :, :, neg, :] = torch.round(far * 4) / 4 + torch.round(K.rnd(N, D, H, int(neg.sum()), C, seed=seed + 4) * 2) / 4
    return y, gamma, mi, ss


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])) + f"k{c[5]}r{int(c[6])}")
def test_pooled_reduce_matches_the_full_size_reduce(hip, case):
    N, D, H, W, C, k, relu = case
    pg = PoolGeom(N, D, H, W, C, k, k, (0, 0, 0))
    y, gamma, mi, ss = _unit(N, D, H, W, C, k)
    do, ho, wo = pg.out_dims
    dout = K.rnd(N, do, ho, wo, C, seed=9)
    with Guarded(DEV) as G:
        yd, ssd, mid, gd, dd = G.put(y), G.put(ss), G.put(mi), G.put(gamma), G.put(dout)
        ref_out = hip.bn_act_pool_fwd(pg, yd, ssd, None, relu)
        got = hip.bn_act_pool_sel_fwd(pg, yd, ssd, relu)
        assert got is not None, "disjoint windows of 4 / 8 positions with C % 4 == 0 are covered"
        out, ysel = got
        assert torch.equal(out.view(torch.int32), ref_out.view(torch.int32)), "forward output differs in some bit"
        # the arg-max rule of the saved pools: maxpool_fwd on the activated tensor (first maximum in scan order; linear position per sample)
        act = hip.bn_act_pool_fwd(PoolGeom(N, D, H, W, C), yd, ssd, None, relu)
        pooled, idx = hip.maxpool_fwd(pg, act, True)
        assert torch.equal(pooled, ref_out)
        want = torch.gather(yd.view(N, D * H * W, C), 1, idx.view(N, -1, C).long()).view(N, do, ho, wo, C)
        assert torch.equal(ysel, want), f"y_sel is not y at the arg-max: {int((ysel != want).sum())} of {want.numel()} differ"
        if relu:
            assert bool((pooled == 0).any()), "no window that is negative throughout in the data"
        assert bool((torch.gather(act.view(N, D * H * W, C), 1, idx.view(N, -1, C).long()).view_as(pooled) == pooled).all())
        dg0, db0, dg1, db1 = (G.alloc((C,), name=n) for n in ("dgamma ref", "dbeta ref", "dgamma", "dbeta"))
        dy0, _ = hip.bn_act_pool_bwd(pg, yd, None, dd, gd, mid, ssd, relu, False, dg0, db0)
        dy1, _ = hip.bn_act_pool_bwd(pg, yd, None, dd, gd, mid, ssd, relu, False, dg1, db1, y_sel=ysel)
        for a, b, what in ((dy1, dy0, "dy"), (dg1, dg0, "dgamma"), (db1, db0, "dbeta")):
            err = (a.double() - b.double()).abs().max().item()
            ref = max(b.double().abs().max().item(), 1e-6)
            print(f"{what}: max abs diff {err:.3e}, rel {err / ref:.3e}")
            assert err <= 2e-5 * ref, f"{what}: rel {err / ref:.3e} > 2e-5"
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: same partitioning, yet not the same bits"
        # ... and against the fp64-accumulating CPU checker, as the existing backward is checked
        dg_ref, db_ref = torch.empty(C), torch.empty(C)
        dy_ref, _ = K.CPU.bn_act_pool_bwd(pg, y, None, dout, gamma, mi, ss, relu, False, dg_ref, db_ref)
        K.close(dy1, dy_ref, 2e-5, "dy vs CPU")
        K.close(dg1, dg_ref, 2e-5, "dgamma vs CPU")
        K.close(db1, db_ref, 2e-5, "dbeta vs CPU")
        G.check()


def test_uncovered_units_are_reported_not_run(hip):
    """Unit windows, windows of 2 positions and channel counts that are no multiple of 4 are not covered: the forward says so (None)
    and the executor keeps the existing path; y_sel with a residual is refused."""
    from rspnet_amd import _lib
    y, ss = K.rnd(2, 4, 6, 6, 64, seed=1).to(DEV), torch.stack([torch.ones(64), torch.zeros(64)]).to(DEV)
    assert hip.bn_act_pool_sel_fwd(PoolGeom(2, 4, 6, 6, 64), y, ss, True) is None
    assert hip.bn_act_pool_sel_fwd(PoolGeom(2, 4, 6, 6, 64, (1, 1, 2), (1, 1, 2), (0, 0, 0)), y, ss, True) is None
    y6, ss6 = K.rnd(2, 4, 6, 6, 6, seed=1).to(DEV), torch.stack([torch.ones(6), torch.zeros(6)]).to(DEV)
    assert hip.bn_act_pool_sel_fwd(PoolGeom(2, 4, 6, 6, 6, (1, 2, 2), (1, 2, 2), (0, 0, 0)), y6, ss6, True) is None
    pg = PoolGeom(2, 4, 6, 6, 64, (1, 2, 2), (1, 2, 2), (0, 0, 0))
    out, ysel = hip.bn_act_pool_sel_fwd(pg, y, ss, True)
    with pytest.raises(_lib.RspError):
        hip.bn_act_pool_bwd(pg, y, y, torch.ones_like(out), torch.ones(64, device=DEV), ss, ss, True, True, None, None, y_sel=ysel)
