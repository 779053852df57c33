"""CPU: the t-SNE rule's numpy fp64 reference against its own properties, the torch composition against the reference, the argument
checks of the C entry points (nothing is launched), the command-line round trip and the monitor's config key."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import tsne_util as tu
from cpu_ops import CpuOps
from rspnet_amd import _lib, ops, tsne


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())      # has no tsne_affinities / tsne_fit: tsne.fit composes the rule from torch ops
    yield
    ops.set_backend(prev)


def test_conditional_rows_hit_the_perplexity():
    x, _ = tu.main_input()
    _, d = tsne.reference_distances(x)
    for perp in (5.0, 20.0, 50.0):
        beta, cond = tsne.calibrate(d, perp)
        pos = np.where(cond > 0, cond, 1.0)
        H = -(cond * np.log(pos)).sum(axis=1)
        assert np.abs(np.exp(H) - perp).max() <= 1e-9 * perp, perp
        assert np.abs(cond.sum(axis=1) - 1).max() <= 1e-12 and (np.diag(cond) == 0).all() and (beta > 0).all()


def test_joint_sums_to_one_and_is_symmetric():
    aff = tu.main_reference().aff
    assert abs(aff.psum - 1.0) <= 1e-12
    assert np.array_equal(aff.p, aff.p.T) and (np.diag(aff.p) == 0).all() and (aff.p >= 0).all()
    assert aff.plogp < 0


def test_a_row_of_equal_distances_stays_finite():
    """Every row of the all-equal distance matrix: H = log(M - 1) at every beta.  Above the perplexity beta doubles 64 times and stays
    finite in fp32 and fp64 alike; the weights are uniform."""
    M = 9
    d = np.full((M, M), 0.75)
    np.fill_diagonal(d, 0)
    for dtype in (np.float64, np.float32):
        beta, cond = tsne.calibrate(d, 3.0, dtype)
        assert np.isfinite(beta).all() and (beta == dtype(2.0) ** 64).all()
        assert np.allclose(cond[~np.eye(M, dtype=bool)], 1.0 / (M - 1), rtol=1e-6, atol=0)
    # a perplexity the row cannot reach (>= M - 1): beta bisects towards 0, finite and uniform
    beta, cond = tsne.calibrate(d, 30.0)
    assert (beta == 2.0 ** -64).all() and np.allclose(cond[~np.eye(M, dtype=bool)], 1.0 / (M - 1))


def test_torch_composition_matches_the_reference():
    """The affinities and single teacher-forced iterations of the fp32 torch composition against the fp64 reference on the same
    fp32 inputs, at the gates."""
    x, _ = tu.main_input()
    ref = tu.main_reference()
    rows, d, beta, p, plogp, psum = tsne.affinities_torch(torch.from_numpy(np.array(x)), tu.PERPLEXITY)
    assert np.array_equal(rows.numpy(), ref.aff.rows)
    tu.close(d.numpy(), ref.aff.d, "torch d")
    own = tsne.affinities_reference(d=d.numpy().astype(np.float64), perplexity=tu.PERPLEXITY)      # calibrated on its own distances
    assert np.abs(beta.numpy() / own.beta - 1).max() <= tu.GATE
    tu.close(p.numpy(), own.p, "torch p")
    assert abs(psum - 1) <= 1e-5 and abs(plogp - own.plogp) <= tu.GATE * abs(own.plogp)
    sched = tu.main_sched()
    p64 = p.numpy().astype(np.float64)
    for t in tu.FORCED:
        y, inc, gains = (np.array(a, dtype=np.float32) for a in ref.states[t])
        lr, mom, ex = (float(v) for v in sched[t][:3])
        g_ref, y_ref, inc_ref, gains_ref, kl_ref = tsne.step_reference(p64, plogp, y.astype(np.float64), inc.astype(np.float64),
                                                                       gains.astype(np.float64), lr, mom, ex)
        ty, ti, tg = torch.from_numpy(y.copy()), torch.from_numpy(inc.copy()), torch.from_numpy(gains.copy())
        g, kl = tsne.step_torch(p, plogp, ty, ti, tg, lr, mom, ex)
        tu.close(g.numpy(), g_ref, f"torch g[{t}]")
        keep = ~tu.knife_edge(g_ref)
        assert np.array_equal(tg.numpy()[keep], tu.expected_gains(g_ref, inc, gains)[keep])
        tu.close(ti.numpy()[keep], inc_ref[keep], f"torch inc[{t}]")
        tu.close(ty.numpy()[keep], y_ref[keep], f"torch y[{t}]")
        assert abs(float(kl) - kl_ref) <= tu.GATE * max(abs(plogp), abs(kl_ref))


def test_fit_on_the_torch_composition(cpu_backend):
    x, lab = tu.clusters(3, 3, 12, 8, 0.3)
    x[5] = 0
    x[17, 2] = np.nan
    res = tsne.fit(torch.from_numpy(x), perplexity=5, iters=60, exag_iters=30, lr=20.0)
    assert res.info["rows_valid"] == 34 and res.info["rows_bad"] == 2 and abs(res.info["psum"] - 1) < 1e-5
    y = res.y.numpy()
    assert np.isnan(y[[5, 17]]).all() and np.isfinite(np.delete(y, [5, 17], axis=0)).all()
    assert np.abs(np.nanmean(y, axis=0)).max() < 1e-5 * np.nanmax(np.abs(y))
    assert np.isnan(res.beta.numpy()[[5, 17]]).all() and res.kl_trace.shape == (60,) and bool(torch.isfinite(res.kl_trace).all())
    assert float(res.kl_trace[-1]) < float(res.kl_trace[30])
    assert tsne.neighbour_purity(y, lab, 5) > 0.6      # (60 iterations: not converged, but far above the 11 / 35 of a random map)
    state = torch.get_rng_state().clone()
    again = tsne.fit(torch.from_numpy(x), perplexity=5, iters=60, exag_iters=30, lr=20.0)
    assert torch.equal(torch.get_rng_state(), state)                       # no global generator is touched
    assert np.array_equal(again.y.numpy(), y, equal_nan=True)
    pca = tsne.fit(torch.from_numpy(x), perplexity=5, iters=5, init="pca")
    assert np.isfinite(np.delete(pca.y.numpy(), [5, 17], axis=0)).all()


def test_limits_are_value_errors(cpu_backend):
    x = torch.ones(4, 6)
    for kw in (dict(perplexity=0.5), dict(perplexity=float("nan")), dict(perplexity=2000), dict(iters=0), dict(iters=10001)):
        with pytest.raises(ValueError):
            tsne.fit(x, **kw)
    for bad in (torch.ones(1, 6), torch.ones(4, 5), torch.ones(16385, 2)):
        with pytest.raises(ValueError):
            tsne.fit(bad, iters=1)
    with pytest.raises(ValueError):
        tsne.fit(x, iters=1, init="spectral")


def test_entry_points_reject_bad_arguments_before_any_launch():
    """RSP_EINVAL / RSP_EWORKSPACE with the entry point's name in rsp_last_error(), on dummy pointers: nothing is dereferenced,
    nothing is launched, no GPU is needed."""
    lib = _lib.load()
    P = ctypes.c_void_p(1 << 20)
    N, D = 65, 34
    need_a, need_f = lib.rsp_tsne_affinities_workspace(N, D), lib.rsp_tsne_fit_workspace(N)
    assert need_a > 4 * N * N and need_f > 0
    assert lib.rsp_tsne_affinities_workspace(1, D) == 0 and lib.rsp_tsne_affinities_workspace(16385, D) == 0
    assert lib.rsp_tsne_affinities_workspace(N, 33) == 0 and lib.rsp_tsne_fit_workspace(1) == 0 and lib.rsp_tsne_fit_workspace(16385) == 0
    assert lib.rsp_tsne_fit_workspace(16384) >= lib.rsp_tsne_fit_workspace(512)

    def aff(N_=N, D_=D, ld=D, perp=30.0, ldp=N, wsb=need_a, x=P):
        return lib.rsp_tsne_affinities(x, ld, N_, D_, perp, P, ldp, P, P, None, P, P, wsb, None)
    for kw in (dict(N_=1), dict(N_=16385, ldp=16385), dict(D_=0), dict(D_=33), dict(D_=4098, ld=4098), dict(ld=D - 2), dict(ld=D + 1),
               dict(perp=0.5), dict(perp=1025.0), dict(perp=float("nan")), dict(perp=float("inf")), dict(ldp=N - 1), dict(x=None),
               dict(x=ctypes.c_void_p((1 << 20) + 4))):
        assert aff(**kw) == -1, kw
        assert lib.rsp_last_error().startswith(b"rsp_tsne_affinities: "), kw
    assert aff(wsb=need_a - 1) == -2 and lib.rsp_last_error() == b"rsp_tsne_affinities: workspace too small"

    def fit(N_=N, ldp=N, first=0, iters=3, wsb=need_f, y=P):
        return lib.rsp_tsne_fit(P, ldp, P, P, N_, P, first, iters, y, P, P, P, P, wsb, None)
    for kw in (dict(N_=1), dict(N_=16385, ldp=16385), dict(ldp=N - 1), dict(first=-1), dict(iters=0), dict(iters=10001), dict(y=None),
               dict(y=ctypes.c_void_p((1 << 20) + 4))):
        assert fit(**kw) == -1, kw
        assert lib.rsp_last_error().startswith(b"rsp_tsne_fit: "), kw
    assert fit(wsb=need_f - 1) == -2 and lib.rsp_last_error() == b"rsp_tsne_fit: workspace too small"


def test_hip_ops_refuse_cpu_tensors():
    be = ops.HipOps()
    with pytest.raises(_lib.RspError):
        be.tsne_affinities(torch.ones(4, 6))


def test_command_line_round_trip(tmp_path, cpu_backend):
    x, lab = tu.clusters(5, 3, 14, 8, 0.3)
    for split, sl in (("train", slice(0, 30)), ("test", slice(30, 42))):
        np.save(tmp_path / f"{split}_fold2_feats.npy", x[sl])
        np.save(tmp_path / f"{split}_fold2_labels.npy", lab[sl])
    out = tsne.main(["--features", str(tmp_path), "--fold", "2", "--perplexity", "5", "--iters", "40", "--seed", "1", "--max-rows", "24",
                     "--size", "96", "--init", "pca"])
    from PIL import Image
    assert Image.open(tmp_path / "tsne_fold2.png").size == (96, 96)
    assert np.load(tmp_path / "tsne_fold2.npy").shape == (24, 2)
    rec = json.load(open(tmp_path / "tsne_fold2.json"))
    assert set(rec) == {"split", "rows", "perplexity", "iters", "seed", "init", "kl", "purity", "info"}
    assert rec["rows"] == 24 and rec["info"]["rows_valid"] == 24 and np.isfinite(rec["kl"]) and 0 <= rec["purity"] <= 1
    assert rec["kl"] == out["kl"] and os.path.getsize(tmp_path / "tsne_fold2.png") > 0


def test_draw_and_purity():
    y = np.array([[0, 0], [0.1, 0], [5, 5], [5.1, 5], [np.nan, 0]])
    lab = np.array([0, 0, 1, 1, 1])
    assert tsne.neighbour_purity(y, lab, 1) == 1.0 and tsne.neighbour_purity(y, lab, 3) == pytest.approx(1 / 3)
    img = tsne.draw(y, lab, 64)
    assert img.size == (64, 64) and img.getpixel((0, 0)) == (255, 255, 255) and len(np.unique(np.asarray(img).reshape(-1, 3), axis=0)) >= 3
    assert tsne.palette(4) == tsne.palette(4) and len(set(tsne.palette(101))) == 101


def test_monitor_config_key():
    assert tsne.TsneMonitor.from_config({}, 4) is None
    assert tsne.TsneMonitor.from_config({"tsne_monitor": {"every": 0}}, 4) is None
    m = tsne.TsneMonitor.from_config({"tsne_monitor": {"every": 3, "perplexity": 5, "iters": 20, "bank_samples": 16}}, 4)
    assert [m.due(e) for e in range(4)] == [False, False, True, True] and m.perplexity == 5.0 and m.bank_samples == 16
    with pytest.raises(ValueError, match="unknown keys"):
        tsne.TsneMonitor.from_config({"tsne_monitor": {"every": 1, "num_clusters": 3}}, 4)
    with pytest.raises(ValueError):
        tsne.TsneMonitor(every=1, num_epochs=1, encoder="x")
    with pytest.raises(ValueError):
        tsne.TsneMonitor(every=1, num_epochs=1, perplexity=0.5)


def test_monitor_refuses_to_run_inside_a_capture(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        tsne.TsneMonitor(every=1, num_epochs=1).run(None, [])
