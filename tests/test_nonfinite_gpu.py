"""GPU: NaN and Inf INSIDE the operands of the training-path kernels (convolutions, BatchNorm, pools, gates, heads, logits, loss,
optimizer), through rspnet_amd.ops.HipOps as tests/test_kernels_gpu.py does.

In every case the non-finite mask of each HIP output equals the expected mask exactly — for the convolutions the footprint
tests/poison_util.py predicts by index arithmetic (validated against conv3d in float64 by tests/test_nonfinite_cpu.py), elsewhere what
CpuOps gives — and outside the mask the values agree with the reference at that op's tolerance in test_kernels_gpu.py (2e-5
convolutions and gradients, 1e-5 / 1e-6 elsewhere), with the same max-norm close() applied to the finite part."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import poison_util as PU
import test_kernels_gpu as K
from cpu_ops import CpuOps
from cpu_ops_eval import CpuOpsEval
from rspnet_amd.ops import ConvGeom, PoolGeom

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = CpuOps()
CPUE = CpuOpsEval()
NAN, INF = float("nan"), float("inf")
rnd, close = K.rnd, K.close


def dev(t):
    return None if t is None else t.to(DEV)


def dev_empty(*shape):
    return torch.empty(*shape, dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def hip():
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    return ops.backend()


def check(out, ref, mask, rtol, what):
    """Non-finite mask of `out` == mask exactly (mask None: the non-finite mask of `ref`, NaN for NaN and equal +-Inf); on the rest
    the max-norm close() of test_kernels_gpu against `ref`."""
    o = out.detach().cpu().float()
    ref = ref.detach().cpu().float()
    assert o.shape == ref.shape, (what, o.shape, ref.shape)
    bad = ~torch.isfinite(o)
    if mask is None:
        want = ~torch.isfinite(ref)
    else:
        want = torch.as_tensor(np.asarray(mask)).expand(o.shape) if not torch.is_tensor(mask) else mask.expand(o.shape)
        assert bool(torch.isfinite(ref[~want]).all()), (what, "reference is not finite outside the mask")
    if not torch.equal(bad, want):
        extra, missing = (bad & ~want).nonzero(), (want & ~bad).nonzero()
        raise AssertionError(f"{what}: non-finite set differs from the expected one: {len(extra)} unexpected (first {extra[:4].tolist()}), "
                             f"{len(missing)} missing (first {missing[:4].tolist()}) of {int(want.sum())} expected")
    if mask is None:
        assert torch.equal(torch.isnan(o), torch.isnan(ref)), f"{what}: NaN where the reference has Inf, or the reverse"
        inf = torch.isinf(ref)
        assert torch.equal(o[inf], ref[inf]), f"{what}: sign of an Inf differs"
    fin = ~want
    if bool(fin.any()):
        close(o[fin], ref[fin], rtol, what)


def check_rows(out, ref, rtol, what):
    """check() against a reference computed on the same (poisoned) inputs, row by row: a row of 1e20 must not hide the others
    behind the max norm."""
    for r in range(ref.shape[0]):
        check(out[r], ref[r], None, rtol, f"{what} row {r}")


# ---- convolution footprints -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_data(case):
    """Seeded operands of a case and the reference from the UN-poisoned tensors, computed once and shared (never modified)."""
    N, D, H, W, Cin, Cout, k, s, p = case
    g = ConvGeom(N, D, H, W, Cin, Cout, k, s, p)
    x = rnd(N, D, H, W, Cin, seed=1)
    if Cin == 4:
        x[..., 3] = 0                                     # the stems' fourth channel is zero padding by contract
    w = rnd(Cout, Cin, *k, seed=2, scale=(Cin * k[0] * k[1] * k[2]) ** -0.5)
    b = rnd(Cout, seed=3)
    y_ref, st_ref = CPU.conv_fwd(g, x, w, b, True)
    dy = rnd(*y_ref.shape, seed=4)
    dx_ref = CPU.conv_dgrad(g, dy, w)
    dw_ref, db_ref = torch.empty_like(w), torch.empty_like(b)
    CPU.conv_wgrad(g, x, dy, dw_ref, db_ref)
    return g, x, w, b, dy, y_ref, st_ref.double().sum(0).float(), dx_ref, dw_ref, db_ref


def _planned(hip, g, which):
    d = g.desc()
    return hip.lib.rsp_conv3d_kernel_name(ctypes.byref(d), which).decode()


def _ran(hip):
    return hip.lib.rsp_last_conv_kernel().decode()


def conv_footprints(hip, case, opts, family):
    """Forward with bias and statistics, dgrad, wgrad with dbias (poisoned x, then poisoned dy), forward with a poisoned weight.
    family: (substring of the forward kernel's name, of the dgrad kernel's), None where the plan's own name is all that is asserted."""
    g, x, w, b, dy, y_ref, st_ref, dx_ref, dw_ref, db_ref = conv_data(case)
    _, px, pdy, pw = PU.conv_poisons(case)
    xp, dyp, wpz = PU.poison(x, px), PU.poison(dy, pdy), PU.poison(w, pw)
    with hip.options(**opts):
        wd, bd = dev(w), dev(b)
        if g.Cin == 4:      # an RGB stem: filters re-packed from their three real channels, as the engine does (the planned name is that instance)
            ps = hip.pack_set([(g, 0, wd[:, :3].contiguous())])
            ps.run()
            wp = ps.packed[0]
        else:
            wp = hip.conv_pack_fwd(g, wd)
        # forward, poisoned x: the union of the footprints, every output channel; every channel's statistics
        y, st = hip.conv_fwd(g, dev(xp), wp, bd, True)
        kf = _ran(hip)
        assert kf == _planned(hip, g, 0), ("fwd", kf)
        m = PU.conv_fwd_x_mask(g, px)
        check(y, y_ref, m, 2e-5, "conv fwd, poisoned x")
        check(st.double().sum(0), st_ref, PU.channels_hit(m)[:, None], 2e-5, "stat partials, poisoned x")
        # dgrad, poisoned dy
        dx = hip.conv_dgrad(g, dev(dyp), wd)
        kd = _ran(hip)
        if g.Cin > 4:       # (a stem's input gradient is not part of a step: test_kernels_gpu checks no name for it either)
            assert kd == _planned(hip, g, 1), ("dgrad", kd)
        check(dx, dx_ref, PU.conv_dgrad_mask(g, pdy), 2e-5, "dgrad, poisoned dy")
        # wgrad + dbias, poisoned x: dw[:, ci, taps], dbias finite
        dw, db = dev_empty(w.shape), dev_empty(b.shape)
        hip.conv_wgrad(g, dev(xp), dev(dy), dw, db)
        kw = _ran(hip)
        assert kw == _planned(hip, g, 2), ("wgrad", kw)
        mw, mb = PU.conv_wgrad_x_mask(g, px)
        check(dw, dw_ref, mw, 2e-5, "wgrad, poisoned x")
        check(db, db_ref, mb, 2e-5, "dbias, poisoned x")
        # wgrad + dbias, poisoned dy: dw[co, :, in-range taps] <= NaN set <= dw[co] (poison_util.conv_wgrad_dy_masks), dbias[co]
        dw, db = dev_empty(w.shape), dev_empty(b.shape)
        hip.conv_wgrad(g, dev(x), dev(dyp), dw, db)
        must, may, mb = PU.conv_wgrad_dy_masks(g, pdy)
        bad = (~torch.isfinite(dw)).cpu().numpy()
        assert not (must & ~bad).any(), ("wgrad, poisoned dy: missing", np.argwhere(must & ~bad)[:4].tolist())
        assert not (bad & ~may).any(), ("wgrad, poisoned dy: outside dw[co]", np.argwhere(bad & ~may)[:4].tolist())
        fin = torch.from_numpy(~may)
        close(dw.cpu()[fin], dw_ref[fin], 2e-5, "wgrad, poisoned dy")
        check(db, db_ref, mb, 2e-5, "dbias, poisoned dy")
        # forward, poisoned weight: must <= NaN set <= may (padding taps may be skipped, masked or multiplied)
        y2, st2 = hip.conv_fwd(g, dev(x), hip.conv_pack_fwd(g, dev(wpz)), bd, True)
        must, may = PU.conv_fwd_w_masks(g, pw)
        bad = (~torch.isfinite(y2)).cpu().numpy()
        assert not (must & ~bad).any(), ("poisoned w: missing", np.argwhere(must & ~bad)[:4].tolist())
        assert not (bad & ~may).any(), ("poisoned w: outside channel co", np.argwhere(bad & ~may)[:4].tolist())
        fin = torch.from_numpy(~may)
        close(y2.cpu()[fin], y_ref[fin], 2e-5, "conv fwd, poisoned w")
        check(st2.double().sum(0), st_ref, PU.channels_hit(may)[:, None], 2e-5, "stat partials, poisoned w")
    assert family[0] in kf and (family[1] is None or family[1] in kd), (kf, kd)
    return kf, kd, kw


# What the instance names show of the family each case is there for (forward, input gradient), under the default plan — at these
# sizes a launch of less than one unit per CU runs on the 32-wide whole-K tiles (`true`: slice-major K walk, `false`: tap-major; VEC = 1:
# the scalar gather; igemm_multi_kernel: the stride-parity classes in one launch) — and under WIDE_OPTS, which turns the two small-launch
# rules off so that the same shapes run on the tiles their column counts select at full size: 128 x 128, the 96-wide slice-major tile,
# the 144-wide tile with its 16-wide half block, 96 columns for 64 + 8.  A K split, padded-tap skipping and depth-major rows do not show
# in a name: there the shape itself (98 rows x 6912 products; N = 3 with depth padding) is what selects them, as in test_kernels_gpu.
C_ = PU.CONV_POISON_CASES
DEFAULT_FAMILY = {
    C_[0]: ("igemm_persist_kernel<128, 32, 4, 1, true", "igemm_persist_kernel<128, 32, 4, 1, true"),
    C_[1]: ("igemm_kernel<128, 64, 2, 2, 1,", "igemm_persist_kernel<128, 96, 4, 1, false"),
    C_[2]: ("igemm_persist_kernel<128, 32, 4, 1, true", "igemm_persist_kernel<128, 32, 4, 1, true"),
    C_[3]: ("igemm_persist_kernel<128, 32, 4, 1, true", "igemm_multi_kernel<128, 64"),
    C_[4]: ("igemm_persist_kernel<128, 32, 4, 1, true", "igemm_persist_kernel<128, 32, 4, 1, true"),
    C_[5]: ("igemm_persist_kernel<128, 32, 4, 1, false", "igemm_persist_kernel<128, 32, 4, 1, false"),
    C_[6]: ("igemm_persist_kernel<128, 32, 4, 1, false", "igemm_multi_kernel<128, 64"),
    C_[7]: ("stem_resident_kernel<", None),
    C_[8]: ("igemm_persist_kernel<128, 32, 4, 1, false", None),
    C_[9]: ("igemm_persist_kernel<128, 32, 4, 1, false", "igemm_persist_kernel<128, 32, 4, 1, false"),
}
WIDE_OPTS = {"narrow32_max_units": 0, "narrow_max_tiles": 0}
WIDE_FAMILY = {
    C_[0]: ("igemm_persist_kernel<128, 128, 2, 2, true", "igemm_persist_kernel<128, 64, 2, 2, true"),
    C_[2]: ("igemm_persist_kernel<128, 96, 4, 1, true", "igemm_persist_kernel<128, 128, 2, 2, true"),
    C_[4]: ("igemm_persist_kernel<128, 128, 2, 2, true", "igemm_persist_kernel<128, 128, 2, 2, true"),
    C_[5]: ("igemm_persist_kernel<128, 144, 4, 1, false", "igemm_persist_kernel<128, 64, 2, 2, false"),
    C_[6]: ("igemm_persist_kernel<128, 96, 4, 1, false", "igemm_multi_kernel<128, 64"),
}


@pytest.mark.parametrize("case", PU.CONV_POISON_CASES, ids=PU.case_id)
def test_conv_footprints(hip, case):
    conv_footprints(hip, case, {}, DEFAULT_FAMILY[case])


@pytest.mark.parametrize("case", list(WIDE_FAMILY), ids=PU.case_id)
def test_conv_footprints_on_the_wide_tiles(hip, case):
    conv_footprints(hip, case, WIDE_OPTS, WIDE_FAMILY[case])


@pytest.mark.parametrize("case", PU.DIRECT_CASES, ids=PU.case_id)
def test_conv_footprints_on_the_direct_kernel(hip, case):
    strided = case[7] != (1, 1, 1)            # (the strided input gradient stays on its parity-class kernel)
    conv_footprints(hip, case, {"direct_max_tiles": PU.DIRECT_MAX_TILES}, ("igemm_direct_kernel", None if strided else "igemm_direct_kernel"))


def test_conv_footprints_on_the_tall_tile(hip):
    conv_footprints(hip, PU.TALL_CASE, {"tall_min_tiles": 2, "narrow32_max_units": 0}, ("<256, 64,", "<256, 64,"))


def test_conv_inf_footprint_carries_the_sign_of_the_weight_tap(hip):
    """One +Inf input next to the three NaN poisons: its footprint is +-Inf with the sign of the weight tap that reads it (an output
    hit by two poisons at once may be NaN: here the footprints are apart, and that is asserted)."""
    case = PU.INF_CASE
    g, x, w, b, dy, y_ref, *_ = conv_data(case)
    _, px, _, _ = PU.conv_poisons(case)
    n, d, h, ww, ci = PU.INF_POISON
    m_nan, m_inf = PU.conv_fwd_x_mask(g, px), PU.conv_fwd_x_mask(g, [PU.INF_POISON])
    assert not (m_nan & m_inf).any() and ci not in {c for *_, c in px}
    want = y_ref.clone()
    want[torch.from_numpy(m_nan)] = NAN
    for (od, oh, ow), (kt, kh, kw) in PU._hits3(g, d, h, ww):
        want[n, od, oh, ow, :] = torch.sign(w[:, ci, kt, kh, kw]) * INF
    assert bool((w[:, ci] != 0).all())
    y, _ = hip.conv_fwd(g, dev(PU.poison(PU.poison(x, px), [PU.INF_POISON], INF)), hip.conv_pack_fwd(g, dev(w)), dev(b), False)
    check(y, want, None, 2e-5, "conv fwd, +Inf and NaN in x")


# ---- BatchNorm and pools ----------------------------------------------------------------------------------------------------------
def _chain(ops, put, empty, pg, y, res, dout, gamma, beta, rm, rv):
    """stat partials (as the convolution epilogue gives them: one tile) -> bn_finalize -> bn_act_pool_fwd -> bn_act_pool_bwd."""
    C = y.shape[-1]
    rows = y.numel() // C
    yy = y.reshape(rows, C).double()
    part = torch.stack([yy.sum(0), (yy * yy).sum(0)], 1).float().unsqueeze(0)
    rm_, rv_ = empty(rm.shape).copy_(rm), empty(rv.shape).copy_(rv)
    mi, ss = ops.bn_finalize(put(part), rows, None, put(gamma), put(beta), 1e-5, 0.1, rm_, rv_)
    yd, rd = put(y), put(res)
    out = ops.bn_act_pool_fwd(pg, yd, ss, rd, True)
    dg, db = empty(C), empty(C)
    dy, dres = ops.bn_act_pool_bwd(pg, yd, rd, put(dout), put(gamma), mi, ss, True, res is not None, dg, db)
    r = {"mean_invstd": mi, "scale_shift": ss, "running_mean": rm_, "running_var": rv_, "out": out, "dy": dy, "dgamma": dg, "dbeta": db}
    if res is not None:
        r["dres"] = dres
    return r


CHAIN_TOL = {"mean_invstd": 1e-5, "scale_shift": 1e-5, "running_mean": 1e-5, "running_var": 1e-5, "out": 1e-6, "dy": 2e-5,
             "dgamma": 2e-5, "dbeta": 2e-5, "dres": 1e-6}


@pytest.mark.parametrize("case,where", [(c, "y") for c in PU.TRAIN_CHAIN_CASES] + [(PU.TRAIN_CHAIN_CASES[2], "residual")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[0])) + f"k{v[1]}")
def test_bn_train_chain(hip, case, where):
    """One NaN in y: NaN in exactly channel c of mean_invstd, scale_shift, the running statistics, the output, dy and dgamma; every
    other channel equals the reference of the un-poisoned tensors.  dbeta and dres of channel c are what torch gives: ReLU's
    backward (threshold_backward) hands the gradient on where its input is NaN, so dz = dout there and dbeta[c] = sum dout is FINITE.
    One NaN in the residual: NaN at that output position only."""
    (N, D, H, W, C), k, use_res = case
    pg = PoolGeom(N, D, H, W, C, k, k, (0, 0, 0))
    c = PU.TRAIN_CHAIN_CHANNEL
    y = rnd(N, D, H, W, C, seed=1) * 2
    res = rnd(N, D, H, W, C, seed=2) if use_res else None
    gamma, beta = rnd(C, seed=3) + 1.5, rnd(C, seed=4) * 0.5
    rm, rv = rnd(C, seed=6), rnd(C, seed=7) + 1.5
    dout = rnd(N, *pg.out_dims, C, seed=5)
    at = (N - 1, D // 2, H // 2, W // 2, c)
    yp, resp = (PU.poison(y, [at]), res) if where == "y" else (y, PU.poison(res, [at]))
    cpu_args = (lambda t: t, lambda *s: torch.empty(*s), pg)
    clean = _chain(CPU, *cpu_args, y, res, dout, gamma, beta, rm, rv)
    same = _chain(CPU, *cpu_args, yp, resp, dout, gamma, beta, rm, rv)
    got = _chain(hip, dev, dev_empty, pg, yp, resp, dout, gamma, beta, rm, rv)
    for name, t in got.items():
        check(t, same[name], None, CHAIN_TOL[name], f"{name} vs the checker on the poisoned tensors")
        if where == "y" and name not in ("dres", "dbeta"):
            chan = np.zeros(t.shape, dtype=bool)
            chan[..., c] = True
            check(t, clean[name], chan, CHAIN_TOL[name], f"{name}: NaN in exactly channel {c}")
    if where == "residual":
        m = np.zeros(got["out"].shape, dtype=bool)
        m[at] = True
        check(got["out"], clean["out"], m, 1e-6, "out: NaN at the poisoned residual's position only")
        for name in ("mean_invstd", "scale_shift", "running_mean", "running_var", "dy", "dgamma", "dbeta", "dres"):
            assert bool(torch.isfinite(got[name]).all()), name


def _finite_bn(pg, relu, seed=0, res=False):
    """y, scale_shift, mean_invstd with every pre-activation at least 1e-4 off zero (a ReLU decision inside the rounding band of
    fmaf against multiply-add is not what these tests are about: tests/test_bn_eval_bwd_gpu.py does the same)."""
    C = pg.C
    y = rnd(pg.N, pg.Di, pg.Hi, pg.Wi, C, seed=61 + seed)
    r = rnd(pg.N, pg.Di, pg.Hi, pg.Wi, C, seed=66 + seed) if res else None
    scale, shift = rnd(C, seed=62 + seed).abs() + 0.5, rnd(C, seed=63 + seed) * 0.3
    z = y * scale + shift + (r if res else 0)
    y = torch.where(z.abs() < 1e-4, y + torch.where(z >= 0, 3e-4, -3e-4) / scale, y)
    ss = torch.stack([scale, shift]).contiguous()
    mi = torch.stack([rnd(C, seed=64 + seed) * 0.3, rnd(C, seed=65 + seed) * 0.4 + 1.0]).contiguous()
    return y, r, ss, mi


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("pg", PU.EVAL_POOL_CASES, ids=PU.pool_id)
def test_bn_act_pool_fwd_and_eval_bwd_with_finite_scale_shift(hip, pg, relu):
    """The eval-mode situation: a NaN activation under finite statistics.  Forward: the output mask is the pool-window footprint
    (first, middle and last element of three different windows).  Backward: NaN positions and gradient routing as torch gives them."""
    y, _, ss, mi = _finite_bn(pg, relu)
    ps = PU.window_poisons(pg)
    yp = PU.poison(y, ps)
    out = hip.bn_act_pool_fwd(pg, dev(yp), dev(ss), None, relu)
    check(out, CPU.bn_act_pool_fwd(pg, y, ss, None, relu), PU.pool_window_mask(pg, ps), 1e-6, "bn_act_pool fwd: window footprint")
    check(out, CPU.bn_act_pool_fwd(pg, yp, ss, None, relu), None, 1e-6, "bn_act_pool fwd vs the checker")
    dout = rnd(*out.shape, seed=5)
    dg_r, db_r = torch.empty(pg.C), torch.empty(pg.C)
    dy_r, _ = CPUE.bn_eval_act_pool_bwd(pg, yp, None, dout, mi, ss, relu, False, dg_r, db_r)
    dg, db = dev_empty(pg.C), dev_empty(pg.C)
    dy, _ = hip.bn_eval_act_pool_bwd(pg, dev(yp), None, dev(dout), dev(mi), dev(ss), relu, False, dg, db)
    check(dy, dy_r, None, 2e-5, "bn eval bwd dy")
    check(dg, dg_r, None, 2e-5, "bn eval bwd dgamma")
    check(db, db_r, None, 2e-5, "bn eval bwd dbeta")
    # the train-mode backward on the same finite statistics routes the same way
    gamma = rnd(pg.C, seed=3) + 1.5
    dg_r, db_r = torch.empty(pg.C), torch.empty(pg.C)
    dy_r, _ = CPU.bn_act_pool_bwd(pg, yp, None, dout, gamma, mi, ss, relu, False, dg_r, db_r)
    dy, _ = hip.bn_act_pool_bwd(pg, dev(yp), None, dev(dout), dev(gamma), dev(mi), dev(ss), relu, False, dg, db)
    check(dy, dy_r, None, 2e-5, "bn train bwd dy")
    check(dg, dg_r, None, 2e-5, "bn train bwd dgamma")
    check(db, db_r, None, 2e-5, "bn train bwd dbeta")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_bn_eval_bwd_with_a_poisoned_residual(hip, relu):
    pg = PoolGeom(2, 3, 5, 5, 64)
    y, r, ss, mi = _finite_bn(pg, relu, seed=10, res=True)
    ps = PU.window_poisons(pg)
    for yp, rp in ((PU.poison(y, ps), r), (y, PU.poison(r, ps))):
        out = hip.bn_act_pool_fwd(pg, dev(yp), dev(ss), dev(rp), relu)
        check(out, CPU.bn_act_pool_fwd(pg, y, ss, r, relu), PU.pool_window_mask(pg, ps), 1e-6, "fwd with residual")
        dout = rnd(*out.shape, seed=5)
        dg_r, db_r = torch.empty(pg.C), torch.empty(pg.C)
        dy_r, dres_r = CPUE.bn_eval_act_pool_bwd(pg, yp, rp, dout, mi, ss, relu, True, dg_r, db_r)
        dg, db = dev_empty(pg.C), dev_empty(pg.C)
        dy, dres = hip.bn_eval_act_pool_bwd(pg, dev(yp), dev(rp), dev(dout), dev(mi), dev(ss), relu, True, dg, db)
        for name, a, b, tol in (("dy", dy, dy_r, 2e-5), ("dres", dres, dres_r, 1e-6), ("dgamma", dg, dg_r, 2e-5), ("dbeta", db, db_r, 2e-5)):
            check(a, b, None, tol, "eval bwd with residual: " + name)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_bn_act_maxpool_fwd_overlapping_window(hip, relu):
    """BatchNorm apply + overlapping 3x3x3 / 2 / 1 max-pool in one pass, with and without kept indices, and the value-only generic
    path of bn_act_pool_fwd: the window footprint of three NaN activations; values and arg-max as apply -> max_pool3d give them."""
    pg = PU.OVERLAP_POOL
    y, _, ss, _ = _finite_bn(pg, relu, seed=20)
    ps = PU.window_poisons(pg)
    yp = PU.poison(y, ps)
    unit = PoolGeom(pg.N, pg.Di, pg.Hi, pg.Wi, pg.C)
    o_clean, _ = CPU.maxpool_fwd(pg, CPU.bn_act_pool_fwd(unit, y, ss, None, relu), True)
    o_ref, _ = CPU.maxpool_fwd(pg, CPU.bn_act_pool_fwd(unit, yp, ss, None, relu), True)
    # the arg-max over the activation's own bits (a ranking inside the rounding band of fmaf against multiply-add is not the point)
    act = hip.bn_act_pool_fwd(unit, dev(yp), dev(ss), None, relu).cpu()
    o_bits, i_ref = CPU.maxpool_fwd(pg, act, True)
    m = PU.pool_window_mask(pg, ps)
    for keep in (True, False):
        fused = hip.bn_act_maxpool_fwd(pg, dev(yp), dev(ss), relu, keep)
        assert fused is not None
        check(fused[0], o_clean, m, 2e-6, f"bn_act_maxpool fwd (keep={keep}): window footprint")
        check(fused[0], o_ref, None, 2e-6, f"bn_act_maxpool fwd (keep={keep}) vs the checker")
        nan = torch.isnan(o_bits)
        assert torch.equal(torch.isnan(fused[0].cpu()), nan) and torch.equal(fused[0].cpu()[~nan], o_bits[~nan])
        if keep:
            assert torch.equal(fused[1].cpu(), i_ref), "arg-max differs from max_pool3d's"
        else:
            assert fused[1] is None
    got = hip.bn_act_pool_fwd(pg, dev(yp), dev(ss), None, relu)
    check(got, o_clean, m, 2e-6, "bn_act_pool fwd, overlapping window: footprint")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_bn_act_gate_fwd(hip, relu):
    """One NaN activation in sample 1: that element of the kept activation, mean[1, c], all of gate[1, :] and all of out[1]."""
    N, D, H, W, C = PU.GATE_FUSED_SHAPE
    pg = PoolGeom(N, D, H, W, C)
    y, _, ss, _ = _finite_bn(pg, relu, seed=30)
    w, b = rnd(C, C, 1, 1, 1, seed=14) * 0.2, rnd(C, seed=15) * 0.1
    at = (1, D // 2, H // 2, W // 2, 9)
    yp = PU.poison(y, [at])
    oc, ac, mc, gc = CPU.bn_act_gate_fwd(pg, y, ss, relu, w, b, True)
    m_a, m_mean = np.zeros(ac.shape, dtype=bool), np.zeros(mc.shape, dtype=bool)
    m_a[at] = True
    m_mean[1, 9] = True
    m_row = np.zeros(gc.shape, dtype=bool)
    m_row[1] = True
    m_o = np.zeros(oc.shape, dtype=bool)
    m_o[1] = True
    for keep_act in (True, False):
        o, a, mean, gate = hip.bn_act_gate_fwd(pg, dev(yp), dev(ss), relu, dev(w), dev(b), keep_act)
        check(o, oc, m_o, 2e-5, "gated output")
        check(mean, mc, m_mean, 2e-5, "gate mean")
        check(gate, gc, m_row, 2e-5, "gate")
        if keep_act:
            check(a, ac, m_a, 1e-6, "kept activation")


def _maxpool_input(pg, kind):
    x = rnd(pg.N, pg.Di, pg.Hi, pg.Wi, pg.C, seed=71)                 # signed: a pool that padded with 0 would show
    if kind == "negative":
        return -(x.abs() + 0.1)
    x[0, ..., 3] = -INF                                                # every window of (sample 0, channel 3) is all -Inf
    x[pg.N - 1, pg.Di - 1, pg.Hi // 2, pg.Wi // 2, 2] = INF            # +Inf, twice in a row: a tie between Infs
    x[pg.N - 1, pg.Di - 1, pg.Hi // 2, pg.Wi // 2 + 1, 2] = INF
    return PU.poison(x, PU.window_poisons(pg))                         # NaN first, in the middle and last in a window


@pytest.mark.parametrize("kind", ["negative", "nonfinite"])
@pytest.mark.parametrize("pg", PU.MAXPOOL_CASES, ids=PU.pool_id)
def test_maxpool_signed_and_nonfinite(hip, pg, kind):
    x = _maxpool_input(pg, kind)
    o_ref, i_ref = CPU.maxpool_fwd(pg, x, True)
    o, idx = hip.maxpool_fwd(pg, dev(x), True)
    o2, none = hip.maxpool_fwd(pg, dev(x), False)
    assert none is None
    if kind == "negative":
        assert bool((o_ref < 0).all())
        assert torch.equal(o.cpu(), o_ref) and torch.equal(o2.cpu(), o_ref)
    else:
        nan = torch.isnan(o_ref)
        assert np.array_equal(nan.numpy(), PU.pool_window_mask(pg, PU.window_poisons(pg)))
        assert bool((o_ref[0, ..., 3][~nan[0, ..., 3]] == -INF).all()) and bool((o_ref == INF).any())
        for got in (o.cpu(), o2.cpu()):
            assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], o_ref[~nan])
    assert torch.equal(idx.cpu(), i_ref)
    dout = rnd(*o_ref.shape, seed=2)
    close(hip.maxpool_bwd(pg, dev(dout), idx), CPU.maxpool_bwd(pg, dout, i_ref), 1e-6, "maxpool bwd")


# ---- gate, heads, logits, loss, glue ----------------------------------------------------------------------------------------------
def test_gate_fwd_bwd(hip):
    N, P, C = PU.GATE_SHAPE
    x = torch.relu(rnd(N, P, 1, 1, C, seed=1))
    w, b = rnd(C, C, 1, 1, 1, seed=2, scale=C ** -0.5), rnd(C, seed=3)
    xp = PU.poison(x, [(1, 7, 0, 0, 9)])
    o_c, m_c, g_c = CPU.gate_fwd(x, w, b)
    o, mean, gate = hip.gate_fwd(dev(xp), dev(w), dev(b))
    m_mean, m_row, m_o = np.zeros((N, C), dtype=bool), np.zeros((N, C), dtype=bool), np.zeros(o_c.shape, dtype=bool)
    m_mean[1, 9] = True
    m_row[1] = True
    m_o[1] = True
    check(o, o_c, m_o, 1e-5, "gate out: sample 1")
    check(mean, m_c, m_mean, 1e-5, "gate mean[1, c]")
    check(gate, g_c, m_row, 1e-5, "gate[1, :]")
    dout = rnd(N, P, 1, 1, C, seed=4)
    o_p, m_p, g_p = CPU.gate_fwd(xp, w, b)
    dw_r, db_r = torch.empty_like(w), torch.empty_like(b)
    dx_r = CPU.gate_bwd(xp, dout, w, m_p, g_p, dw_r, db_r)
    dw, db = dev_empty(w.shape), dev_empty(b.shape)
    dx = hip.gate_bwd(dev(xp), dev(dout), dev(w), mean, gate, dw, db)
    check(dx, dx_r, None, 2e-5, "gate dx")
    check(dw, dw_r, None, 2e-5, "gate dw")
    check(db, db_r, None, 2e-5, "gate db")
    assert bool(torch.isfinite(dx[0]).all()) and bool(torch.isfinite(dx[2]).all()) and bool(torch.isnan(dx[1]).all())


def test_gate_saturates_to_exactly_zero_and_one(hip):
    N, P, C = PU.GATE_SHAPE
    x = torch.relu(rnd(N, P, 1, 1, C, seed=1))
    w = rnd(C, C, 1, 1, 1, seed=2, scale=C ** -0.5) * 1e-3
    b = torch.cat([torch.full((C // 2,), 200.0), torch.full((C - C // 2,), -200.0)])
    o, mean, gate = hip.gate_fwd(dev(x), dev(w), dev(b))
    assert torch.equal(gate.cpu(), torch.cat([torch.ones(N, C // 2), torch.zeros(N, C - C // 2)], 1))
    assert torch.equal(o.cpu()[..., :C // 2], x[..., :C // 2]) and float(o[..., C // 2:].abs().max()) == 0.0


def _five_rows(C, seed):
    """Rows: one NaN, all zero, one +Inf, finite elements whose sum of squares overflows fp32, ordinary."""
    x = rnd(5, C, seed=seed)
    x[0, 3] = NAN
    x[1] = 0
    x[2, C - 1] = INF
    x[3] = x[3].sign() * 1e20
    return x


def test_head_fwd_bwd_rows(hip):
    B, P, C, dim = 5, 8, 512, 128
    rows = _five_rows(C, 1)
    feat = rnd(B, P, 1, 1, C, seed=2) * 0.5
    feat[0, 2, 0, 0, 3] = NAN
    feat[1] = 0
    feat[2, P - 1, 0, 0, C - 1] = INF
    feat[3] = rows[3].view(1, 1, 1, C).expand(P, 1, 1, C)
    w1, w2 = rnd(dim, C, seed=2, scale=C ** -0.5), rnd(dim, C, seed=3, scale=C ** -0.5)
    b1, b2 = torch.zeros(dim), torch.zeros(dim)              # (no bias: the all-zero row stays all zero in front of the normalisation)
    ref = CPU.head_fwd(feat, w1, b1, w2, b2)
    d = [dev(t) for t in (feat, w1, b1, w2, b2)]
    got = hip.head_fwd(*d)
    for a, r, n in zip(got[:3], ref[:3], ("head out1", "head out2", "pooled")):
        check_rows(a, r, 1e-5, n)
    check_rows(got[3].transpose(0, 1), ref[3].transpose(0, 1), 1e-5, "raw")
    assert bool(torch.isfinite(ref[3][:, 3]).all()) and bool(torch.isinf((ref[3][:, 3] ** 2).sum(1)).all())      # the overflow row is one
    g1, g2 = rnd(B, dim, seed=6), rnd(B, dim, seed=7)
    refs = [torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2)]
    dfeat_r = CPU.head_bwd(g1, g2, ref[2], ref[3], w1, w2, tuple(feat.shape), *refs)
    outs = [dev_empty(t.shape) for t in refs]
    dfeat = hip.head_bwd(dev(g1), dev(g2), got[2], got[3], d[1], d[3], tuple(feat.shape), *outs)
    check_rows(dfeat, dfeat_r, 2e-5, "dfeat")
    for a, r, n in zip(outs, refs, ("dw1", "db1", "dw2", "db2")):
        check(a, r, None, 2e-5, n)


def test_mlp_head_pieces_rows(hip):
    B, C, dim = 5, 512, 128
    feat = rnd(B, 2, 3, 3, C, seed=1)
    feat[0, 1, 1, 1, 3] = NAN
    feat[1] = 0
    feat[2, 0, 2, 2, C - 1] = -INF
    feat[3] = 1e30
    check_rows(hip.spatial_mean_fwd(dev(feat)), CPU.spatial_mean_fwd(feat), 1e-6, "spatial mean")
    x, w, b = _five_rows(C, 3), rnd(dim, C, seed=4, scale=C ** -0.5), rnd(dim, seed=5)
    for relu in (True, False):
        y_ref = CPU.linear_fwd(x, w, b, relu)
        y = hip.linear_fwd(dev(x), dev(w), dev(b), relu)
        check_rows(y, y_ref, 1e-5, f"linear fwd relu={relu}")
        assert bool(torch.isnan(y_ref[0]).all())
    r = _five_rows(dim, 7)
    check_rows(hip.l2norm_fwd(dev(r)), torch.nn.functional.normalize(r, dim=1), 1e-6, "l2norm")
    g = rnd(5, dim, seed=8)
    check_rows(hip.l2norm_bwd(dev(r), dev(g)), CPU.l2norm_bwd(r, g), 2e-5, "l2norm bwd")


def test_linear_bwd_through_a_nan_activation(hip):
    """ReLU's backward on the kept output, as torch's threshold_backward: the gradient is dropped where y <= 0 and handed on where
    y is NaN (y = relu(z) is NaN exactly where z is)."""
    B, C, dim = 5, 512, 128
    x, w = rnd(B, C, seed=3), rnd(dim, C, seed=4, scale=C ** -0.5)
    y = CPU.linear_fwd(x, w, rnd(dim, seed=5), True)
    y[0, 5], y[4, 100] = NAN, INF
    dy = rnd(B, dim, seed=6)
    dw_r, db_r = torch.empty_like(w), torch.empty(dim)
    dx_r = CPU.linear_bwd(x, y, dy, w, True, dw_r, db_r)
    yy = y.clone().requires_grad_(True)                      # torch's own op, not the checker's restatement
    (dz_t,) = torch.autograd.grad(torch.relu(yy), yy, dy)
    assert float(dz_t[0, 5]) == float(dy[0, 5]) and torch.equal(dx_r, dz_t @ w)
    dw, db = dev_empty(w.shape), dev_empty(dim)
    dx = hip.linear_bwd(dev(x), dev(y), dev(dy), dev(w), True, dw, db)
    check(dx, dx_r, None, 2e-5, "linear dx")
    check(dw, dw_r, None, 2e-5, "linear dw")
    check(db, db_r, None, 2e-5, "linear db")


def test_logits_rows_and_columns(hip):
    B, Kq, dim = 4, 64, 128
    f = [torch.nn.functional.normalize(rnd(B, dim, seed=i), dim=1) for i in range(6)]
    queue = torch.nn.functional.normalize(rnd(dim, Kq, seed=9), dim=0)
    ref = CPU.logits_fwd(*f, queue, 1 / 0.07)
    fp = list(f)
    fp[0] = PU.poison(f[0], [(2, 5)])                         # qA row 2
    qp = PU.poison(queue, [(3, 7)])                           # queue column 7 = logits column 8
    out = hip.logits_fwd(*[dev(t) for t in fp], dev(qp), 1 / 0.07)
    m = np.zeros((B, Kq + 1), dtype=bool)
    m[2, :] = True
    m[:, 8] = True
    check(out[0], ref[0], m, 1e-5, "logits1")
    check(out[1], ref[1], m, 1e-5, "logits2")
    check(out[2], ref[2], np.zeros((B, 1), dtype=bool), 1e-5, "l_pos_M")
    check(out[3], ref[3], np.zeros((B, 1), dtype=bool), 1e-5, "l_neg_M")


@pytest.mark.parametrize("what", ["nan_logit", "nan_margin_pos", "nan_margin_neg", "inf_positive_logit"])
def test_loss_nonfinite(hip, what):
    B, K1 = 4, 65
    l1, l2 = rnd(B, K1, seed=1) * 5, rnd(B, K1, seed=2) * 5
    lp, ln = rnd(B, 1, seed=3) * 3, rnd(B, 1, seed=4) * 3
    if what == "nan_logit":
        l1[2, 3] = NAN
    elif what == "nan_margin_pos":
        lp[1] = NAN
    elif what == "nan_margin_neg":
        ln[3] = NAN
    else:
        l1[1, 0] = INF
    ref = CPU.loss_fwd_bwd(l1, l2, lp, ln, 2.0, 0.7, 1.3)
    out = hip.loss_fwd_bwd(dev(l1), dev(l2), dev(lp), dev(ln), 2.0, 0.7, 1.3)
    assert bool(torch.isnan(ref[0][0]))
    if what == "nan_logit":
        assert torch.equal(torch.isnan(ref[1]).all(1), torch.tensor([False, False, True, False])) and bool(torch.isfinite(ref[2]).all())
    if what.startswith("nan_margin"):
        assert bool(torch.isnan(ref[0][2])) and bool(torch.isfinite(ref[0][1]))
    check(out[0], ref[0], None, 1e-5, "losses")
    for a, r, n in zip(out[1:], ref[1:], ("dlogits1", "dlogits2", "dlpos", "dlneg")):
        check(a, r, None, 2e-5, n)


N_ELT = 4099
SPOTS = [(0, NAN), (4095, INF), (4098, -INF)]      # first element, last of the 16-byte part, last of the scalar tail


def _spotted(t):
    t = t.clone()
    for i, v in SPOTS:
        t[i] = v
    return t


def _only_spots(t, what, all_three=True):
    bad = (~torch.isfinite(t.cpu())).nonzero().flatten().tolist()
    want = [i for i, _ in SPOTS]
    assert (bad == want) if all_three else (len(bad) > 0 and set(bad) <= set(want)), (what, bad)


@pytest.mark.parametrize("op", ["relu_fwd", "relu_bwd", "sigmoid_fwd", "sigmoid_bwd", "add"])
def test_eltwise_nonfinite(hip, op):
    """NaN, +Inf and -Inf at elements 0, 4095 and 4098 of the operand the op hands on (relu_bwd / sigmoid_bwd: the gradient).  The
    non-finite elements afterwards are those the checker gives — all three, but for relu(-Inf) = 0 and sigmoid(+-Inf) = 1 / 0 —
    and the rest equals the reference of the un-poisoned operands."""
    a, b = rnd(N_ELT, seed=1), rnd(N_ELT, seed=2)
    if op == "sigmoid_bwd":
        a = torch.sigmoid(a)
    if op == "relu_bwd":
        for i, _ in SPOTS:
            a[i] = 0.5
    binary = op in ("relu_bwd", "sigmoid_bwd", "add")
    ap, bp = (a, _spotted(b)) if op in ("relu_bwd", "sigmoid_bwd") else (_spotted(a), b)
    clean = CPU.eltwise(op, a, b if binary else None)
    ref = CPU.eltwise(op, ap, bp if binary else None)
    out = hip.eltwise(op, dev(ap), dev(bp) if binary else None)
    check(out, ref, None, 1e-6, op)
    _only_spots(out, op, all_three=op not in ("relu_fwd", "sigmoid_fwd"))
    keep = torch.ones(N_ELT, dtype=torch.bool)
    keep[[i for i, _ in SPOTS]] = False
    close(out.cpu()[keep], clean[keep], 1e-6, op + " elsewhere")
    if op == "relu_fwd":
        assert bool(torch.isnan(out[0])) and float(out[4095]) == INF and float(out[4098]) == 0.0


def test_eltwise_relu_bwd_through_a_nonfinite_activation(hip):
    """NaN, +Inf and -Inf in the ACTIVATION operand of relu_bwd, against torch's own backward of relu (not the checker's restatement):
    the gradient is handed on at the NaN and at +Inf, dropped at -Inf; the result is finite everywhere."""
    a, b = _spotted(rnd(N_ELT, seed=1)), rnd(N_ELT, seed=2)
    aa = a.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(torch.relu(aa), aa, b)
    assert float(want[0]) == float(b[0]) and float(want[4095]) == float(b[4095]) and float(want[4098]) == 0.0
    assert torch.equal(CPU.eltwise("relu_bwd", a, b), want)
    out = hip.eltwise("relu_bwd", dev(a), dev(b)).cpu()
    assert torch.equal(out, want)


def test_momentum_and_sgd_nonfinite(hip):
    k, q = rnd(N_ELT, seed=1), rnd(N_ELT, seed=2)
    kp = _spotted(k)
    kd = dev_empty(N_ELT).copy_(kp)
    hip.momentum_update(kd, dev(q), 0.999)
    CPU.momentum_update(kp, q, 0.999)
    check(kd, kp, None, 1e-7, "momentum")
    _only_spots(kd, "momentum")
    p, g, buf = rnd(N_ELT, seed=3), rnd(N_ELT, seed=4), rnd(N_ELT, seed=5)
    gp = _spotted(g)
    for first in (True, False):
        pd, bd = dev_empty(N_ELT).copy_(p), dev_empty(N_ELT).copy_(buf)
        hip.sgd_step(pd, dev(gp), bd, 0.05, 0.9, 1e-4, 1.0, first)
        p2, b2 = p.clone(), buf.clone()
        CPU.sgd_step(p2, gp, b2, 0.05, 0.9, 1e-4, 1.0, first)
        check(pd, p2, None, 1e-6, f"sgd p (first={first})")
        check(bd, b2, None, 1e-6, f"sgd buf (first={first})")
        _only_spots(pd, "sgd p")
        _only_spots(bd, "sgd buf")
