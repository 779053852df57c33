"""GPU: rsp_tsne_affinities and rsp_tsne_fit (csrc/tsne.hip) against the numpy fp64 reference of rspnet_amd.tsne, at the project's
per-kernel gate of 2e-5 relative to the tensor's largest magnitude.  The figures each check measured are in profiles/tsne_tests.txt."""
import json
import random
import types

import numpy as np
import pytest
import torch

import tsne_util as tu
from guarded import Guarded
from rspnet_amd import ops, tsne

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def fresh_state(N, y0):
    return dev(np.array(y0, dtype=np.float32)), torch.zeros(N, 2, device=DEV), torch.ones(N, 2, device=DEV)


@pytest.fixture(scope="module")
def main_aff():
    """The affinities of the 300-row input from the kernel, once for the tests that iterate on them."""
    x, _ = tu.main_input()
    aff = ops.backend().tsne_affinities(dev(x), tu.PERPLEXITY)
    info = tsne.read_info(aff.info)
    return aff, info, aff.pmat.cpu().numpy().astype(np.float64)


# ---- 1. affinities ---------------------------------------------------------------------------------------------------------------
# (N, D, perplexity, extra row pitch): the tile edges of the distance kernel (64 x 128), of the pair kernel (64) and of the k loop (32)
AFF_CASES = [(2, 2, 2.0, 0), (3, 34, 2.0, 0), (63, 2, 5.0, 0), (64, 130, 30.0, 0), (65, 34, 30.0, 2), (127, 34, 5.0, 0),
             (129, 130, 30.0, 0), (257, 34, 30.0, 0), (65, 34, 64.0, 0)]


@pytest.mark.parametrize("case", AFF_CASES, ids=str)
def test_affinities_match_the_reference(case):
    N, D, perp, gap = case
    x, _ = tu.clusters(N + D, 3, (N + 2) // 3, D, 0.5)
    x = x[:N]
    wide = torch.full((N, D + gap), float("nan"), device=DEV)
    wide[:, :D] = dev(x)
    aff = ops.backend().tsne_affinities(wide[:, :D], perp, want_dmat=True)
    info = tsne.read_info(aff.info)
    assert info["rows_valid"] == N and info["rows_bad"] == 0 and aff.rows.cpu().tolist() == list(range(N))
    d, p, beta = aff.dmat.cpu().numpy(), aff.pmat.cpu().numpy(), aff.beta.cpu().numpy()
    assert np.array_equal(d, d.T) and np.array_equal(p, p.T) and (np.diag(p) == 0).all() and (np.diag(d) == 0).all()
    _, d_ref = tsne.reference_distances(x)
    tu.close(d, d_ref, f"{case} d", scale=max(float(d_ref.max()), 1.0))      # (d = 2 - 2 s: the error is that of s, of magnitude 1)
    own = tsne.affinities_reference(d=d.astype(np.float64), perplexity=perp)      # calibrated on the kernel's own distances
    assert np.isfinite(beta).all() and np.isfinite(p).all()
    if perp >= N - 1:
        # Out of reach: H < log(M - 1) <= log(perplexity) at every beta, so beta bisects towards 0.  Near 0, H = log(M - 1) -
        # beta^2 Var_j(d_ij) / 2 + ...; fp32 cannot tell that from log(M - 1) once beta^2 Var / 2 is below about an ulp of H (2^-22 at
        # most here), and from there on the rounding of H decides the steps: beta stops somewhere below beta sigma ~ 1e-3 (fp64 does
        # the same near 1e-8).  Bound, with a margin of 4 on that estimate: beta sigma <= 4e-3.  The weights exp(-beta (d - m)) are then
        # uniform to beta (max - min) of the row, which is what "uniform" is held to.
        off = ~np.eye(N, dtype=bool)
        rows_d = np.where(off, d.astype(np.float64), np.nan)
        sigma, spread = np.nanstd(rows_d, axis=1), np.nanmax(rows_d, axis=1) - np.nanmin(rows_d, axis=1)
        print(f"tsne-figure {case} beta sigma: {float((beta * sigma).max()):.3e} (bound 4e-03), beta: {beta.min():.3e} .. {beta.max():.3e}")
        assert (beta > 0).all() and (beta * sigma <= 4e-3).all()
        assert np.allclose(p[off], 1.0 / (N * (N - 1)), rtol=2 * float((beta * spread).max()) + 1e-6, atol=0)
        assert np.allclose(own.p[off], 1.0 / (N * (N - 1)), rtol=1e-6, atol=0)      # (fp64 stops the same way, near beta sigma = 1e-8)
    else:
        err = float(np.abs(beta / own.beta - 1).max())
        print(f"tsne-figure {case} beta: {err:.3e} (gate {tu.GATE:.0e})")
        assert err <= tu.GATE
        tu.close(p, own.p, f"{case} p")
    assert abs(info["psum"] - 1.0) <= 1e-5 and abs(info["psum"] - p.astype(np.float64).sum()) <= 1e-12
    assert abs(info["plogp"] - own.plogp) <= tu.GATE * abs(own.plogp)


# ---- 2. teacher-forced iterations ------------------------------------------------------------------------------------------------
def reference_step_on(p64, plogp, state, sched_row):
    y, inc, gains = (np.array(a, dtype=np.float32) for a in state)      # the fp32 inputs the kernel gets
    lr, mom, ex = (float(v) for v in sched_row[:3])
    out = tsne.step_reference(p64, plogp, y.astype(np.float64), inc.astype(np.float64), gains.astype(np.float64), lr, mom, ex)
    return (y, inc, gains), (lr, mom, ex), out


@pytest.mark.parametrize("t", tu.FORCED)
def test_one_iteration_from_the_reference_state(t, main_aff):
    """One rsp_tsne_fit iteration from the fp64 trajectory's state before iteration t, against the fp64 step on the same fp32 state,
    the kernel's own p and plogp.  kl is a sum of three terms of magnitude ~10 that nearly cancel: its error is gated relative to
    the largest of them."""
    aff, info, p64 = main_aff
    ref, sched = tu.main_reference(), tu.main_sched()
    (y, inc, gains), (lr, mom, ex), (g_ref, y_ref, inc_ref, gains_ref, kl_ref) = reference_step_on(p64, info["plogp"], ref.states[t], sched[t])
    yd, incd, gd = dev(y), dev(inc), dev(gains)
    kl = ops.backend().tsne_fit(aff, dev(sched), t, 1, yd, incd, gd)
    y_k, inc_k, g_k = yd.cpu().numpy(), incd.cpu().numpy(), gd.cpu().numpy()
    keep = ~tu.knife_edge(g_ref)
    assert np.array_equal(g_k[keep], tu.expected_gains(g_ref, inc, gains)[keep])
    # the gradient the stored inc implies; inc' is rounded to fp32, which the division by lr gains' carries into g: that floor is added
    g_imp = tu.implied_gradient(inc_k, inc, g_k, lr, mom)
    floor = float((2.0 ** -23 * (np.abs(inc_k) + mom * np.abs(inc)) / (lr * g_k))[keep].max())
    err = float(np.abs(g_imp - g_ref)[keep].max())
    print(f"tsne-figure forced[{t}] g: {err / np.abs(g_ref).max():.3e} (gate {tu.GATE:.0e}, rounding floor {floor / np.abs(g_ref).max():.1e})")
    assert err <= tu.GATE * np.abs(g_ref).max() + floor
    tu.close(inc_k[keep], inc_ref[keep], f"forced[{t}] inc", scale=np.abs(inc_ref).max())
    tu.close(y_k[keep], y_ref[keep], f"forced[{t}] y", scale=np.abs(y_ref).max())
    tu.close(float(kl[0]), kl_ref, f"forced[{t}] kl", scale=max(abs(info["plogp"]), abs(kl_ref)))


# ---- 3. free run -----------------------------------------------------------------------------------------------------------------
def test_five_free_iterations(main_aff):
    aff, info, p64 = main_aff
    sched, y0 = tu.main_sched(), tu.main_y0()
    y = np.array(y0, dtype=np.float64)
    inc, gains = np.zeros_like(y), np.ones_like(y)
    excluded = np.zeros(y.shape, dtype=bool)
    kls, gains32 = [], np.ones(y.shape, dtype=np.float32)
    for t in range(5):
        before = inc
        g, y, inc, gains, kl = tsne.step_reference(p64, info["plogp"], y, inc, gains, *(float(v) for v in sched[t][:3]))
        gains32 = tu.expected_gains(g, before, gains32)      # the reference's branches, the fp32 arithmetic
        excluded |= np.abs(g) < tu.KNIFE * np.abs(g).max()
        kls.append(kl)
    assert excluded.mean() <= tu.MAX_EXCLUDED
    yd, incd, gd = fresh_state(300, y0)
    kl = ops.backend().tsne_fit(aff, dev(sched), 0, 5, yd, incd, gd)
    keep = ~excluded
    assert np.array_equal(gd.cpu().numpy()[keep], gains32[keep])
    tu.close(yd.cpu().numpy()[keep], y[keep], "free y after 5", scale=np.abs(y).max())
    tu.close(incd.cpu().numpy()[keep], inc[keep], "free inc after 5", scale=np.abs(inc).max())
    tu.close(kl.cpu().numpy(), np.array(kls), "free kl", scale=abs(info["plogp"]))


# ---- 4. the whole fit -------------------------------------------------------------------------------------------------------------
def test_whole_fit_separates_the_clusters():
    x, lab = tu.main_input()
    ref = tu.main_reference()
    res = tsne.fit(dev(x), tu.PERPLEXITY, tu.FIT_ITERS, tu.EXAG, tu.EXAG_ITERS, lr=tu.LR, seed=0)
    kl = res.kl_trace.cpu().numpy()
    purity = tsne.neighbour_purity(res.y, lab, 10)
    print(f"tsne-figure whole fit: purity@10 {purity:.4f}, final KL {kl[-1]:.5f}, reference {ref.kl[-1]:.5f}, kl[250] {kl[250]:.5f}")
    assert res.info["rows_valid"] == 300 and np.isfinite(kl).all()
    assert purity >= 0.95
    assert kl[-1] < kl[250]
    assert kl[-1] <= 1.3 * ref.kl[-1]
    assert float(res.y.abs().max()) > 1 and float(res.y.mean(dim=0).abs().max()) < 1e-4 * float(res.y.abs().max())


# ---- 5. invalid rows ---------------------------------------------------------------------------------------------------------------
def test_invalid_rows_take_part_in_nothing():
    invalid_rows_case(132, [0, 70, 131])      # one 256-row trip of the compaction


def test_invalid_rows_take_part_in_nothing_over_two_trips():
    invalid_rows_case(300, [0, 63, 64, 255, 256, 299])      # (255, 256: the last lane of the first trip, the first lane of the second)


def invalid_rows_case(N, bad):
    D, iters = 34, 4
    x, _ = tu.clusters(9, 3, N // 3, D, 0.5)
    for n, i in enumerate(bad):      # a zero row, a row with a NaN, a row with an Inf, in turn
        if n % 3 == 0:
            x[i] = 0
        else:
            x[i, 3 if n % 3 == 1 else 5] = np.nan if n % 3 == 1 else np.inf
    good = np.delete(np.arange(N), bad)
    rng = np.random.default_rng(2)
    y0 = (rng.standard_normal((N, 2)) * 1e-4).astype(np.float32)
    sched = dev(tsne.schedule(iters, 20.0, 12.0, 2))
    be = ops.backend()
    outs = []
    for xs, ys in ((x, y0), (x[good], y0[good])):
        aff = be.tsne_affinities(dev(xs), 10.0, want_dmat=True)
        n = xs.shape[0]
        y, inc, gains = dev(ys), torch.full((n, 2), 0.0, device=DEV), torch.full((n, 2), 1.0, device=DEV)
        if n == N:      # marks no arithmetic produces in the rows that must stay untouched
            for t_ in (y, inc, gains):
                t_.view(torch.int32)[bad] = -7
        kl = be.tsne_fit(aff, sched, 0, iters, y, inc, gains)
        outs.append((aff, tsne.read_info(aff.info), y, inc, gains, kl))
    (fa, fi, fy, finc, fg, fkl), (ca, ci, cy, cinc, cg, ckl) = outs
    M = N - len(bad)
    assert fi["rows_valid"] == M and fi["rows_bad"] == len(bad) and ci["rows_valid"] == M and ci["rows_bad"] == 0
    assert fa.rows.cpu().tolist() == list(good) + [-1] * len(bad) and (fi["plogp"], fi["psum"]) == (ci["plogp"], ci["psum"])
    assert torch.equal(bits(fa.pmat[:M, :M]), bits(ca.pmat)) and torch.equal(bits(fa.dmat[:M, :M]), bits(ca.dmat))
    assert torch.equal(bits(fa.beta[:M]), bits(ca.beta)) and bool(torch.isnan(fa.beta[M:]).all())
    assert bool((fa.pmat[M:] == 0).all()) and bool((fa.pmat[:, M:] == 0).all())
    g = dev(good)
    for full, compact in ((fy, cy), (finc, cinc), (fg, cg)):
        assert torch.equal(bits(full[g]), bits(compact))
        assert bool((full.view(torch.int32)[bad] == -7).all())
    assert torch.equal(bits(fkl), bits(ckl)) and bool(torch.isfinite(fkl).all())


# ---- 6. determinism and capture ------------------------------------------------------------------------------------------------------
def test_same_bits_over_runs_and_under_capture():
    N, D, iters = 129, 34, 3
    x, _ = tu.clusters(4, 3, 43, D, 0.5)
    x[7] = 0
    xd, sched = dev(x), dev(tsne.schedule(iters, 20.0, 12.0, 2))
    y0 = (np.random.default_rng(5).standard_normal((N, 2)) * 1e-4).astype(np.float32)
    be = ops.backend()

    def run(y, inc, gains):
        aff = be.tsne_affinities(xd, 10.0, want_dmat=True)
        kl = be.tsne_fit(aff, sched, 0, iters, y, inc, gains)
        return [aff.pmat, aff.rows, aff.beta, aff.dmat, aff.info, kl]
    state = fresh_state(N, y0)
    eager = run(*state) + list(state)
    for _ in range(2):
        again = fresh_state(N, y0)
        for a, b in zip(eager, run(*again) + list(again)):
            assert torch.equal(bits(a), bits(b))
    cap_state = fresh_state(N, y0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = run(*cap_state)
    for _ in range(2):
        for t_, src in zip(cap_state, fresh_state(N, y0)):
            t_.copy_(src)
        for t_ in cap:
            t_.view(torch.uint8).fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, cap + list(cap_state)):
            assert torch.equal(bits(a), bits(b))


# ---- 7. guarded memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [65, 129])
def test_guarded_memory(N):
    """Every operand, output and workspace inside 0xFF-filled allocations at the 8-byte alignment the header promises (x with row
    pitch D + 2, the gap is NaN), one invalid row present: no byte outside them changes, x and the schedule do not change, every
    float output is written, the gap's NaNs reach no output, the invalid row's state keeps its bytes."""
    D, iters = 34, 3
    x, _ = tu.clusters(N, 3, (N + 2) // 3, D, 0.5)
    x = x[:N]
    x[N // 2] = 0
    be = ops.backend()
    y0 = (np.random.default_rng(N).standard_normal((N, 2)) * 1e-4).astype(np.float32)
    with Guarded(DEV, skew=8) as G:
        wide = G.alloc((N, D + 2), name="wide x")
        wide[:, :D] = dev(x)
        xd = wide[:, :D]
        before = wide.clone()
        sched = G.put(torch.from_numpy(tsne.schedule(iters, 20.0, 12.0, 2)))
        y, inc, gains = G.alloc((N, 2), name="y"), G.alloc((N, 2), name="inc"), G.alloc((N, 2), name="gains")
        y.copy_(dev(y0))
        inc.zero_()
        gains.fill_(1.0)
        for t_ in (y, inc, gains):
            t_.view(torch.int32)[N // 2] = -7
        assert xd.data_ptr() % 16 == 8 and y.data_ptr() % 16 == 8 and sched.data_ptr() % 16 == 8
        aff = be.tsne_affinities(xd, 10.0, want_dmat=True)
        G.check()
        kl = be.tsne_fit(aff, sched, 0, iters, y, inc, gains)
        G.check()
        assert torch.equal(bits(wide), bits(before)) and bool((wide.view(torch.int32)[:, D:] == -1).all())
        assert [blk.kind for blk in G.blocks].count("workspace") >= 1
        info = tsne.read_info(aff.info)
        assert info["rows_valid"] == N - 1 and info["rows_bad"] == 1 and abs(info["psum"] - 1) <= 1e-5
        assert bool(torch.isfinite(kl).all()) and bool(torch.isfinite(aff.pmat).all()) and bool(torch.isfinite(aff.dmat).all())
        keep = torch.arange(N, device=DEV) != N // 2
        for t_ in (y, inc, gains):
            assert bool(torch.isfinite(t_[keep]).all()) and bool((t_.view(torch.int32)[N // 2] == -7).all())


# ---- 8. a NaN in y0 ------------------------------------------------------------------------------------------------------------------
def test_a_nan_in_the_map_propagates_and_nothing_faults(main_aff):
    aff, _, _ = main_aff
    y0 = np.array(tu.main_y0())
    y0[17, 1] = np.nan
    y, inc, gains = fresh_state(300, y0)
    kl = ops.backend().tsne_fit(aff, dev(tu.main_sched()), 0, 3, y, inc, gains)
    torch.cuda.synchronize()
    assert bool(torch.isnan(kl).all()) and bool(torch.isnan(y).all())


def test_resumed_fit_continues_the_trajectory(main_aff):
    aff, _, _ = main_aff
    sched, be = dev(tu.main_sched()), ops.backend()
    a, b = fresh_state(300, tu.main_y0()), fresh_state(300, tu.main_y0())
    kl = be.tsne_fit(aff, sched, 0, 6, *a)
    kl2 = torch.cat([be.tsne_fit(aff, sched, 0, 2, *b), be.tsne_fit(aff, sched, 2, 4, *b)])
    assert torch.equal(bits(kl), bits(kl2)) and all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


# ---- 9. the monitor ------------------------------------------------------------------------------------------------------------------
def test_monitor_run_leaves_the_model_and_the_generators_alone(tmp_path):
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory
    torch.manual_seed(3)
    model = ModelFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=DEV)
    net = model.module
    net.train()
    net.encoder_k.eval()
    mon = tsne.TsneMonitor(every=1, num_epochs=1, perplexity=5, iters=40, bank_samples=24, batch_size=4)
    (bank,) = mon.build_loaders(16, 32, DEV, seed=0)
    before = {n: t_.clone() for n, t_ in net.state_dict().items()}
    flags = [m.training for m in net.modules()]
    states = (random.getstate(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(DEV).clone())
    out = mon.run(model, bank, str(tmp_path / "map"), image_size=64)
    assert set(out) == {"kl", "purity", "n_bank", "bad_rows", "seconds"}
    assert out["n_bank"] == 24 and out["bad_rows"] == 0 and np.isfinite(out["kl"]) and 0 <= out["purity"] <= 1
    assert np.load(tmp_path / "map.npy").shape == (24, 2) and (tmp_path / "map.png").stat().st_size > 0
    after = net.state_dict()
    assert list(after) == list(before)
    for n, t_ in after.items():
        assert torch.equal(t_, before[n]), n
    assert [m.training for m in net.modules()] == flags
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    assert torch.equal(torch.cuda.get_rng_state(DEV), states[2])
    again = mon.run(model, bank)
    assert all(again[k] == out[k] for k in out if k != "seconds")


def _args(tmp_path, keys, name):
    cfg = json.load(open("rspnet_amd/config/pretrain/c3d.json"))
    cfg.update(batch_size=4, num_epochs="2", log_interval=2)
    cfg["moco"]["k"] = 64
    cfg["spatial_transforms"]["size"] = 32
    cfg.update(keys)
    (tmp_path / name).mkdir()
    p = tmp_path / name / "cfg.json"
    json.dump(cfg, open(p, "w"))
    exp = tmp_path / name / "exp"
    return types.SimpleNamespace(config=str(p), ext_config=None, experiment_dir=str(exp), load_checkpoint=None, load_model=None,
                                 debug=False, world_size=1, seed=0, no_scale_lr=False, steps_per_epoch=3, run_dir=str(exp / "run_0_t"),
                                 cont=False)


def test_pretext_driver_with_and_without_the_monitor(tmp_path):
    """Two epochs, the monitor every second one: its scalars and files belong to the second epoch only.  Without the key no line
    carries such a scalar, no file is written and the backend's tsne calls are never made; both runs train the same model."""
    from rspnet_amd.pretrain import main_worker
    be = ops.backend()
    calls = []
    inner = be.tsne_affinities

    def counted(x, *a, **kw):
        calls.append(tuple(x.shape))
        return inner(x, *a, **kw)
    be.tsne_affinities = counted
    try:
        keys = {"tsne_monitor": {"every": 2, "perplexity": 5, "iters": 40, "bank_samples": 24, "batch_size": 4}}
        main_worker(0, _args(tmp_path, keys, "with"), "")
        with_calls = list(calls)
        del calls[:]
        main_worker(0, _args(tmp_path, {}, "without"), "")
        without_calls = list(calls)
    finally:
        del be.tsne_affinities
    runs = {name: tmp_path / name / "exp" / "run_0_t" for name in ("with", "without")}
    lines = {name: [json.loads(l) for l in open(runs[name] / "scalars.jsonl")] for name in runs}
    assert len(lines["with"]) == 2 and len(lines["without"]) == 2
    first, second = lines["with"]
    assert not any(k.startswith("tsne_") for k in first)
    assert sorted(k for k in second if k.startswith("tsne_")) == ["tsne_kl", "tsne_purity"]
    assert np.isfinite(second["tsne_kl"]) and 0 <= second["tsne_purity"] <= 1
    assert (runs["with"] / "tsne_epoch1.png").exists() and np.load(runs["with"] / "tsne_epoch1.npy").shape == (24, 2)
    assert not (runs["with"] / "tsne_epoch0.png").exists() and not list(runs["without"].glob("tsne_*"))
    assert len(with_calls) == 1 and with_calls[0][0] == 24 and without_calls == []
    assert not any(k.startswith("tsne_") for rec in lines["without"] for k in rec)
    for a, b in zip(lines["with"], lines["without"]):
        assert {k: v for k, v in a.items() if not k.startswith("tsne_")} == b
    a = torch.load(tmp_path / "with" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    b = torch.load(tmp_path / "without" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n
