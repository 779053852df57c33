"""GPU: the key passes' conv1 leaves its stem kernel pooled (ops.stem_pooled_fwd + ops.bn_act_minmax_fwd).

A pass that keeps nothing for a backward reads conv1's output only through BatchNorm -> ReLU -> MaxPool(1,2,2).  The pooled stem
instance writes the maximum and the minimum of the raw output over each window instead of the output; the follower applies
BatchNorm + ReLU to the one the scale's sign selects.  Both are exact (a correctly rounded fma and ReLU are monotone), so every
comparison here is `==` with NaNs in the same places — against the three existing ops (conv_fwd, bn_finalize, bn_act_pool_fwd) on
the same device, no tolerance; the statistic partials are compared bit for bit.

Shapes: N=2, D=3, H=W in {16, 20, 36}, 3 -> 4 input channels, 64 filters: whole 8 x 16 patches, partial ones (20 = 16 + 4 columns,
2 x 8 + 4 rows), and patch borders inside the frame.  Every operand sits in guarded memory (tests/guarded.py): a store outside
either pooled output, or an element of them left unwritten, fails Guarded.check()."""
import pytest
import torch

import test_kernels_gpu as K
from guarded import Guarded
from rspnet_amd import engine
from rspnet_amd.ops import ConvGeom, PoolGeom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COUT = 64
NAN, INF, BIG = float("nan"), float("inf"), 3.0e38


@pytest.fixture(scope="module")
def hip():
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    return ops.backend()


def _geom(H, W, N=2, D=3):
    return ConvGeom(N, D, H, W, 4, COUT, (3, 3, 3), (1, 1, 1), (1, 1, 1), Cin_alg=3)


def _operands(H, W, nonfinite):
    """x (N,D,H,W,4) with a zero fourth channel, three-channel filters, bias.  nonfinite: the centre tap of channel 0 is +-4 (sign by
    filter parity), so an input of +-3e38 overflows to +-inf at exactly that output position in every filter — both signs of
    infinity in every class of scale — and stays finite around it; an input NaN makes its whole 3x3x3 neighbourhood NaN.  The marks
    sit on window corners and on both sides of the patch borders (rows 7|8, columns 15|16), and in the frame's corners."""
    g = _geom(H, W)
    x = K.rnd(g.N, g.Di, H, W, 4, seed=11)
    x[..., 3] = 0
    w = K.rnd(COUT, 3, 3, 3, 3, seed=12, scale=0.2)
    b = K.rnd(COUT, seed=13)
    if nonfinite:
        w[0::2, 0, 1, 1, 1] = 4.0
        w[1::2, 0, 1, 1, 1] = -4.0
        hs = (7, 8) if H > 8 else (H - 1,)
        ws = (15, 16) if W > 16 else (W - 2, W - 1)
        for i, (h_, w_) in enumerate([(h_, w_) for h_ in hs for w_ in ws] + [(0, 0), (H - 1, W - 1), (1, 2), (2, 1)]):
            x[i % g.N, i % g.Di, h_, w_, 0] = BIG if i % 2 == 0 else -BIG
        x[1, 2, min(7, H - 1), min(15, W - 1), 1] = NAN      # a NaN blob across a patch corner
        x[0, 0, H - 1, 0, 2] = NAN                           # ... and in a frame corner
    return g, x, w, b


def _same(a, b, what):
    """== with NaNs in the same places (the sign of a zero may differ)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    an, bn = torch.isnan(a), torch.isnan(b)
    assert torch.equal(an, bn), f"{what}: NaNs in different places ({int(an.sum())} vs {int(bn.sum())})"
    ok = (a == b) | an
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements differ"


def _window_ref(y, fn):
    """max / min over the (1,2,2) windows of y (N,D,H,W,C), NaN if the window holds one (torch.amax / amin propagate NaN)."""
    N, D, H, W, C = y.shape
    return fn(y.view(N, D, H // 2, 2, W // 2, 2, C), dim=(3, 5))


def _scale_shift(C=COUT, seed=21):
    """[2][C] with positive, negative and exactly zero scales"""
    sc = K.rnd(C, seed=seed) + 0.25
    sc[3::7] = 0.0
    sc[5::7] = -sc[5::7].abs() - 0.1
    return torch.stack([sc, K.rnd(C, seed=seed + 1) * 0.5]).contiguous()


@pytest.mark.parametrize("three", [True, False], ids=["rgb-filters", "4ch-filters"])
@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nonfinite"])
@pytest.mark.parametrize("HW", [16, 20, 36])
def test_pooled_stem_and_follower_equal_the_three_ops(hip, HW, nonfinite, three):
    g, x, w, b = _operands(HW, HW, nonfinite)
    pg = PoolGeom(g.N, g.Di, HW, HW, COUT, (1, 2, 2), (1, 2, 2), (0, 0, 0))
    gamma, beta = K.rnd(COUT, seed=3) + 1.5, K.rnd(COUT, seed=4) * 0.5
    gamma[2::5] = -gamma[2::5]
    gamma[4::5] = 0.0
    with Guarded(DEV) as G:
        xd, bd = G.put(x), G.put(b)
        if three:
            ps = hip.pack_set([(g, 0, G.put(w))])
            ps.run()
            wp = ps.packed[0]
        else:
            wp = hip.conv_pack_fwd(g, G.put(torch.cat([w, torch.zeros(COUT, 1, 3, 3, 3)], 1)))
        y, st = hip.conv_fwd(g, xd, wp, bd, True)
        got = hip.stem_pooled_fwd(g, xd, wp, bd)
        assert got is not None, "the pooled instance must cover this shape"
        assert hip.lib.rsp_last_conv_kernel().decode().endswith(", 3, true>" if three else ", 4, true>")
        ymax, ymin, st2 = got
        assert torch.equal(st.view(torch.int32), st2.view(torch.int32)), "statistic partials differ in some bit"
        if nonfinite:
            assert bool(torch.isnan(y).any()) and bool((y == INF).any()) and bool((y == -INF).any())
        _same(ymax, _window_ref(y, torch.amax), "window maximum")
        _same(ymin, _window_ref(y, torch.amin), "window minimum")
        # the follower against bn_act_pool_fwd on the full-size output: hand-made scales of both signs and zero (also where the
        # statistics of a non-finite output would make every scale NaN) ...
        for relu in (True, False):
            ss = G.put(_scale_shift())
            ref = hip.bn_act_pool_fwd(pg, y, ss, None, relu)
            out = hip.bn_act_minmax_fwd(ymax, ymin, ss, relu)
            _same(out, ref, f"follower, relu={relu}")
            if nonfinite and relu:
                zero = (ss[0] == 0).cpu()
                assert bool(torch.isnan(ref.cpu()[..., zero]).any()) and bool((_window_ref(y, torch.amin).cpu()[..., zero] == -INF).any()), \
                    "the case '-inf under a zero scale' is not in the data"
        # ... and the unit as the engine runs it: conv_fwd + bn_finalize + bn_act_pool_fwd against the two new ops around bn_finalize
        gd, be_ = G.put(gamma), G.put(beta)
        _, ss_ref = hip.bn_finalize(st, g.rows, bd, gd, be_, 1e-5, 0.1, None, None)
        _, ss_new = hip.bn_finalize(st2, g.rows, bd, gd, be_, 1e-5, 0.1, None, None)
        assert torch.equal(ss_ref.view(torch.int32), ss_new.view(torch.int32))
        if not nonfinite:
            assert bool((ss_ref[0] > 0).any()) and bool((ss_ref[0] < 0).any()) and bool((ss_ref[0] == 0).any())
        _same(hip.bn_act_minmax_fwd(ymax, ymin, ss_new, True), hip.bn_act_pool_fwd(pg, y, ss_ref, None, True), "whole unit")
        # into a channel slice of a wider tensor, as a unit with `into` writes
        wide = G.alloc(tuple(ymax.shape[:4]) + (COUT + 24,), name="wide out")
        hip.bn_act_minmax_fwd(ymax, ymin, ss_new, True, out=wide[..., 8:8 + COUT])
        _same(wide[..., 8:8 + COUT], hip.bn_act_pool_fwd(pg, y, ss_ref, None, True), "whole unit into a slice")
        bits = wide.view(torch.int32)
        assert bool((bits[..., :8] == -1).all()) and bool((bits[..., 8 + COUT:] == -1).all()), "a store outside the channel slice"
        G.check()


def _stem_plan(seed=31):
    torch.manual_seed(seed)
    conv, bn = torch.nn.Conv3d(3, COUT, 3, padding=1).to(DEV), torch.nn.BatchNorm3d(COUT).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(K.rnd(COUT, seed=5) + 0.3)
        bn.weight[1::6] = 0.0
        bn.bias.copy_(K.rnd(COUT, seed=6) * 0.5)
    node = engine.ConvBN(conv, bn, 0, 1, (3, 3, 3), (1, 1, 1), (1, 1, 1), relu=True, pool=((1, 2, 2), (1, 2, 2)))
    return engine.Plan([node], 0, 1)


def _key_pass(plan, x, on, calls=None):
    """A forward that keeps nothing, with the switch on or off; calls: list that receives what stem_pooled_fwd returned."""
    from rspnet_amd import ops
    be = ops.backend()
    saved, inner = engine.STEM_POOLED, be.stem_pooled_fwd

    def spy(*a, **kw):
        r = inner(*a, **kw)
        calls.append(r is not None)
        return r
    engine.STEM_POOLED = on
    if calls is not None:
        be.stem_pooled_fwd = spy
    try:
        out, ctx = engine.run_forward(plan, x, engine.PackedWeights(), keep=False, training=True)
    finally:
        engine.STEM_POOLED = saved
        if calls is not None:
            del be.stem_pooled_fwd
    assert ctx is None
    return out


@pytest.mark.parametrize("H,W,taken", [(16, 16, True), (20, 36, True), (16, 15, False), (15, 16, False)])
def test_engine_takes_the_path_on_even_frames_and_falls_back_on_odd_ones(hip, H, W, taken):
    plan = _stem_plan()
    x = torch.zeros(2, 3, H, W, 4, device=DEV)
    x[..., :3] = K.rnd(2, 3, H, W, 3, seed=7).to(DEV)
    calls = []
    on = _key_pass(plan, x, True, calls)
    off = _key_pass(plan, x, False)
    assert calls == ([True] if taken else []), (calls, "odd frames never reach the op: the executor itself falls back")
    assert on.shape == (2, 3, H // 2, W // 2, COUT)
    _same(on, off, "key-pass unit, switch on vs off")
    # a pass that keeps its state for a backward never takes it
    calls = []
    saved, be = engine.STEM_POOLED, hip
    inner = be.stem_pooled_fwd
    be.stem_pooled_fwd = lambda *a, **kw: calls.append(1) or inner(*a, **kw)
    try:
        engine.run_forward(plan, x, engine.PackedWeights(), keep=True, training=True)
    finally:
        del be.stem_pooled_fwd
    assert not calls


def test_c3d_key_pass_feature_is_equal_with_the_switch_on_and_off(hip):
    """C3D at B=2, 16 x 32 x 32: the feature of a forward that keeps nothing (what the key encoder computes), == either way."""
    from rspnet_amd.models.c3d import C3D
    torch.manual_seed(3)
    model = C3D(with_classifier=False).to(DEV)
    model.train()
    x = torch.zeros(2, 16, 32, 32, 4, device=DEV)
    x[..., :3] = K.rnd(2, 16, 32, 32, 3, seed=8).to(DEV)
    plan = model.plan()
    calls = []
    on = _key_pass(plan, x, True, calls)
    off = _key_pass(plan, x, False)
    assert calls == [True]
    assert on.shape == off.shape == (2, 2, 2, 2, 512)
    _same(on, off, "C3D key-pass feature")
