"""No GPU: the reference side of tests/test_nonfinite_gpu.py.

(1) The footprints tests/poison_util.py predicts by index arithmetic against the NaN masks of torch.nn.functional.conv3d / max_pool3d
in float64 — forward, and the two gradients through autograd — for every convolution case of the GPU module; exact, but for the two
places where conv3d multiplies a NaN by an explicit padding zero (a poisoned weight in the forward, a poisoned dy in the weight
gradient: there the prediction is a lower bound and the poisoned channel an upper one).  (2) CpuOps, the
contract the HIP kernels are held to, itself hands non-finite values on: relu, max-pool (value and index), F.normalize, clamp(min=0),
batch_norm.  (3) The caps on the GPU module's inputs: in every case the expected non-finite set is non-empty, covers at most half of
each output, and leaves at least 100 elements to compare by value."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import poison_util as PU
from cpu_ops import CpuOps
from rspnet_amd.ops import ConvGeom, PoolGeom

CPU = CpuOps()
NAN = float("nan")
ALL_CONV = PU.CONV_POISON_CASES + [PU.TALL_CASE]


def _rnd(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _conv64(g, x, w):
    return F.conv3d(x.permute(0, 4, 1, 2, 3), w, None, g.s, g.p).permute(0, 2, 3, 4, 1)


def _nan(t):
    return torch.isnan(t).numpy()


@pytest.mark.parametrize("case", ALL_CONV, ids=PU.case_id)
def test_conv_footprints_match_conv3d_in_float64(case):
    g, px, pdy, pw = PU.conv_poisons(case)
    x = _rnd(g.N, g.Di, g.Hi, g.Wi, g.Cin, seed=1)
    w = _rnd(g.Cout, g.Cin, *g.k, seed=2)
    dy = _rnd(g.N, *g.out_dims, g.Cout, seed=3)
    # forward, poisoned x
    assert np.array_equal(_nan(_conv64(g, PU.poison(x, px), w)), PU.conv_fwd_x_mask(g, px))
    # forward, poisoned w: must <= NaN set <= may (conv3d multiplies its explicit padding zeros by the NaN)
    must, may = PU.conv_fwd_w_masks(g, pw)
    got = _nan(_conv64(g, x, PU.poison(w, pw)))
    assert not (must & ~got).any() and not (got & ~may).any()
    assert must.any() and (must <= may).all()
    # dgrad / wgrad through autograd
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(_conv64(g, xr, wr), [xr, wr], PU.poison(dy, pdy))
    assert np.array_equal(_nan(dx), PU.conv_dgrad_mask(g, pdy))
    must, may, mb = PU.conv_wgrad_dy_masks(g, pdy)
    got = _nan(dw)
    # (the weight gradient's matrix product meets the explicit padding zeros of the unfolded input: conv3d marks the padded taps of
    # the poisoned output channels too — in float64 all of them, in float32 at some shapes — never another channel, never less than
    # the prediction)
    assert not (must & ~got).any() and not (got & ~may).any()
    dw32 = torch.empty(g.Cout, g.Cin, *g.k)
    CPU.conv_wgrad(g, x.float(), PU.poison(dy, pdy).float(), dw32, None)
    assert not (must & ~_nan(dw32)).any() and not (_nan(dw32) & ~may).any()
    assert np.array_equal(_nan(PU.poison(dy, pdy).sum(dim=(0, 1, 2, 3))), mb)
    xr = PU.poison(x, px).requires_grad_(True)
    (dw,) = torch.autograd.grad(_conv64(g, xr, wr), [wr], dy)
    mw, mb = PU.conv_wgrad_x_mask(g, px)
    assert np.array_equal(_nan(dw), mw) and not mb.any()


@pytest.mark.parametrize("case", [c for c in ALL_CONV if c[1] * c[2] * c[3] > 25], ids=PU.case_id)
def test_one_interior_poison_gives_cout_times_taps(case):
    """One poisoned interior element of a stride-1 convolution is read once by every tap: Cout x taps NaNs, taps x Cin in dgrad."""
    N, D, H, W, Cin, Cout, k, s, p = case
    g = ConvGeom(N, D, H, W, Cin, Cout, k, (1, 1, 1), p)
    pos = (N - 1, D // 2, H // 2, W // 2, 1)
    taps = k[0] * k[1] * k[2]
    # taps that read the position, per axis: tap kt reads it from output coordinate o = c + p - kt, which must exist.  Every tap
    # does in all cases but two: the two-frame one (D = 2 under a 3-deep kernel: each frame is read by 2 of the 3 depth taps) and
    # the 7-deep stem over 5 frames (5 of 7)
    per_axis = [sum(0 <= c + pp - kt <= n + 2 * pp - kk for kt in range(kk)) for kk, pp, c, n in zip(k, p, pos[1:4], (D, H, W))]
    reading = per_axis[0] * per_axis[1] * per_axis[2]
    assert (reading == taps) == (case not in (PU.CONV_POISON_CASES[4], PU.CONV_POISON_CASES[8])), (per_axis, k)
    m = PU.conv_fwd_x_mask(g, [pos])
    x = _rnd(N, D, H, W, Cin, seed=4)
    w = _rnd(Cout, Cin, *k, seed=5)
    got = _nan(_conv64(g, PU.poison(x, [pos]), w))
    assert np.array_equal(got, m)
    assert int(got.sum()) == Cout * reading


POOLS = [PoolGeom(1, 3, 4, 9, 8, (3, 3, 3), (1, 1, 1), (1, 1, 1)), PoolGeom(2, 4, 7, 7, 83, (1, 3, 3), (1, 2, 2), (0, 1, 1)),
         PoolGeom(2, 2, 6, 6, 64, (2, 2, 2), (2, 2, 2), (0, 0, 0)), PoolGeom(1, 5, 9, 11, 20, (3, 3, 3), (2, 2, 2), (1, 1, 1))]


@pytest.mark.parametrize("pg", POOLS, ids=lambda pg: f"{pg.N}x{pg.Di}x{pg.Hi}x{pg.Wi}x{pg.C}k{pg.k}")
def test_pool_window_footprint_matches_max_pool3d(pg):
    x = _rnd(pg.N, pg.Di, pg.Hi, pg.Wi, pg.C, seed=6).float()
    ps = [(0, 0, 0, 0, 0), (pg.N - 1, pg.Di - 1, pg.Hi - 1, pg.Wi - 1, pg.C - 1), (0, pg.Di // 2, pg.Hi // 2, pg.Wi // 2, 1)]
    o, idx = CPU.maxpool_fwd(pg, PU.poison(x, ps), True)
    assert np.array_equal(_nan(o), PU.pool_window_mask(pg, ps))


# ---- CpuOps hands non-finite values on --------------------------------------------------------------------------------------------
def test_cpu_ops_relu_and_batch_norm_propagate_nan():
    a = torch.tensor([NAN, -1.0, 2.0, float("inf"), float("-inf")])
    r = CPU.eltwise("relu_fwd", a)
    assert torch.isnan(r[0]) and r[1:].tolist() == [0.0, 2.0, float("inf"), 0.0]
    pg = PoolGeom(1, 1, 2, 2, 4)
    y = torch.ones(1, 1, 2, 2, 4)
    y[0, 0, 1, 0, 2] = NAN
    ss = torch.stack([torch.ones(4), torch.zeros(4)])
    for relu in (True, False):
        o = CPU.bn_act_pool_fwd(pg, y, ss, None, relu)
        assert torch.equal(torch.isnan(o), torch.isnan(y))
    assert torch.isnan(CPU.linear_fwd(torch.tensor([[NAN, 1.0]]), torch.ones(3, 2), None, True)).all()
    # batch_norm of a channel with a NaN: statistics, scale / shift and running statistics of that channel, and only of it
    yy = y.reshape(4, 4).double()
    part = torch.stack([yy.sum(0), (yy * yy).sum(0)], 1).float().unsqueeze(0)
    rm, rv = torch.zeros(4), torch.ones(4)
    mi, sc = CPU.bn_finalize(part, 4, None, torch.ones(4), torch.zeros(4), 1e-5, 0.1, rm, rv)
    want = torch.tensor([False, False, True, False])
    for t in (mi[0], mi[1], sc[0], sc[1], rm, rv):
        assert torch.equal(torch.isnan(t), want)
    o = F.batch_norm(y.reshape(4, 4), None, None, training=True)
    assert torch.equal(torch.isnan(o), want.expand(4, 4))


@pytest.mark.parametrize("where", ["first", "middle", "last", "two"])
def test_cpu_ops_maxpool_keeps_a_nan_anywhere_in_the_window(where):
    pg = PoolGeom(1, 1, 1, 5, 1, (1, 1, 5), (1, 1, 5), (0, 0, 0))
    x = torch.tensor([1.0, 5.0, 3.0, 2.0, 4.0]).view(1, 1, 1, 5, 1)
    at = {"first": [0], "middle": [2], "last": [4], "two": [1, 3]}[where]
    for i in at:
        x[0, 0, 0, i, 0] = NAN
    o, idx = CPU.maxpool_fwd(pg, x, True)
    assert torch.isnan(o).all() and int(idx) == at[-1]          # (v > max) || isnan(v): the last NaN holds the window
    dx = CPU.maxpool_bwd(pg, torch.full((1, 1, 1, 1, 1), 7.0), idx)
    assert dx.flatten().tolist() == [7.0 if i == at[-1] else 0.0 for i in range(5)]
    # all -Inf: value -Inf, index of the first element; +Inf wins
    o, idx = CPU.maxpool_fwd(pg, torch.full((1, 1, 1, 5, 1), float("-inf")), True)
    assert float(o) == float("-inf") and int(idx) == 0


def test_cpu_ops_normalize_clamp_and_relu_backward():
    r = torch.tensor([[1.0, NAN, 2.0], [0.0, 0.0, 0.0], [1.0, float("inf"), 2.0], [3e19, 3e19, 3e19], [1.0, 2.0, 3.0]])
    y = CPU.l2norm_fwd(r)
    assert torch.isnan(y[0]).all() and torch.equal(y[1], torch.zeros(3)) and torch.isfinite(y[4]).all()
    assert torch.equal(torch.isnan(y[2]), torch.tensor([False, True, False]))
    g = CPU.l2norm_bwd(r, torch.ones_like(r))
    assert torch.isnan(g[0]).all() and torch.isnan(g[2]).all() and torch.isfinite(g[[1, 3, 4]]).all()
    # clamp(min=0) of a NaN margin term: the ranking loss and the total are NaN, the gradient of that row is 0
    l1, l2 = torch.zeros(3, 4), torch.zeros(3, 4)
    lp, ln = torch.tensor([[1.0], [NAN], [0.5]]), torch.zeros(3, 1)
    losses, d1, d2, dp, dn = CPU.loss_fwd_bwd(l1, l2, lp, ln, 2.0, 1.0, 1.0)
    assert torch.isnan(losses[0]) and torch.isfinite(losses[1]) and torch.isnan(losses[2])
    assert dp.flatten().tolist() == [-1 / 3, 0.0, -1 / 3] or torch.allclose(dp.flatten(), torch.tensor([-1 / 3, 0.0, -1 / 3]))
    assert torch.isfinite(d1).all() and torch.isfinite(dn).all()
    # a NaN logit: that row of dlogits and the loss, nothing else
    l1[1, 2] = NAN
    losses, d1, d2, dp, dn = CPU.loss_fwd_bwd(l1, l2, torch.ones(3, 1), ln, 2.0, 1.0, 1.0)
    assert torch.isnan(losses[0]) and torch.equal(torch.isnan(d1).all(1), torch.tensor([False, True, False])) and torch.isfinite(d2).all()
    # ReLU's backward hands the gradient on at a NaN input (threshold_backward drops it where the input is <= 0)
    pg = PoolGeom(1, 1, 1, 3, 1)
    yv = torch.tensor([NAN, -1.0, 2.0]).view(1, 1, 1, 3, 1)
    ss = torch.stack([torch.ones(1), torch.zeros(1)])
    from cpu_ops_eval import CpuOpsEval
    dy, _ = CpuOpsEval().bn_eval_act_pool_bwd(pg, yv, None, torch.full((1, 1, 1, 3, 1), 5.0), ss, ss, True, False, None, None)
    assert dy.flatten().tolist() == [5.0, 0.0, 5.0]


# ---- caps on the GPU module's inputs ----------------------------------------------------------------------------------------------
def _caps(what, mask, need_100=True):
    n, bad = mask.size, int(mask.sum())
    assert bad > 0, (what, "expected non-finite set is empty")
    assert 2 * bad <= n, (what, bad, n)
    if need_100:
        assert n - bad >= 100, (what, n - bad)


@pytest.mark.parametrize("case", ALL_CONV, ids=PU.case_id)
def test_caps_of_the_convolution_cases(case):
    """Per-channel vectors of fewer than 200 entries (dbias, the summed statistics) cannot leave 100 finite ones: there the cap is
    the half alone.  The statistics under a poisoned x are the one exception to the half: a forward footprint covers every output
    channel, so all of them are non-finite by construction (tests/test_nonfinite_gpu.py asserts exactly that)."""
    g, px, pdy, pw = PU.conv_poisons(case)
    _caps("fwd", PU.conv_fwd_x_mask(g, px))
    assert PU.channels_hit(PU.conv_fwd_x_mask(g, px)).all()
    _caps("dgrad", PU.conv_dgrad_mask(g, pdy))
    mw, mb = PU.conv_wgrad_x_mask(g, px)
    _caps("wgrad(x)", mw)
    must, may, mb = PU.conv_wgrad_dy_masks(g, pdy)
    _caps("wgrad(dy) must", must)
    _caps("wgrad(dy) may", may)
    _caps("dbias", mb, need_100=g.Cout >= 200)
    must, may = PU.conv_fwd_w_masks(g, pw)
    _caps("fwd(w) must", must)
    _caps("fwd(w) may", may)
    _caps("stats(w)", PU.channels_hit(may), need_100=g.Cout >= 200)
    if case == PU.INF_CASE:
        _caps("fwd(+Inf)", PU.conv_fwd_x_mask(g, [PU.INF_POISON]))


def test_caps_of_the_pool_and_batchnorm_cases():
    for shape, k, _res in PU.TRAIN_CHAIN_CASES:
        m = np.zeros(shape, dtype=bool)
        m[..., PU.TRAIN_CHAIN_CHANNEL] = True                   # the whole channel, in y's dims (the pooled output: the same share)
        _caps(("train chain", shape), m)
    for pg in PU.EVAL_POOL_CASES + [PU.OVERLAP_POOL] + PU.MAXPOOL_CASES:
        _caps(("pool footprint", pg), PU.pool_window_mask(pg, PU.window_poisons(pg)))
    N, D, H, W, C = PU.GATE_FUSED_SHAPE
    assert N >= 3                                               # one poisoned sample of the gated unit: a third of the output
    N, P, C = PU.GATE_SHAPE
    assert N == 3 and (N - 1) * P * C >= 100


def test_window_poisons_sit_first_middle_and_last_in_three_different_windows():
    for pg in PU.EVAL_POOL_CASES:
        ps = PU.window_poisons(pg)
        nwin = pg.k[0] * pg.k[1] * pg.k[2]
        seen, wins = [], set()
        for n, d, h, w, c in ps:
            off = ((d % pg.s[0]) * pg.k[1] + (h % pg.s[1])) * pg.k[2] + (w % pg.s[2])
            seen.append(off)
            wins.add((n, d // pg.s[0], h // pg.s[1], w // pg.s[2], c))
        assert seen == [0, nwin // 2, nwin - 1] and len(wins) == 3, (pg, seen)
