"""GPU: rsp_kmeans_fit / rsp_kmeans_assign / rsp_contingency against the fp64 rule (cluster.kmeans_reference) -- one iteration across
the tile edges, equality with the cosine search, whole fits exactly and iteration by iteration, empty clusters, non-finite values,
determinism and capture, guarded memory, the contingency table, bad arguments -- and the pretext driver's monitor."""
import ctypes
import json
import random
import types

import numpy as np
import pytest
import torch

import cluster_util as cu
from guarded import FILL, Guarded
from knn_util import feats
from rspnet_amd import _lib, cluster, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def run_fit(x, cent, iters):
    """(KmeansResult, info dict, final centroids) of one rsp_kmeans_fit call from a copy of ``cent``."""
    c = dev(cent) if isinstance(cent, np.ndarray) else cent.clone()
    r = ops.backend().kmeans_fit(x, c, iters)
    return r, cluster.read_info(r.info), c


def one_iteration(x, cent, sim_ref, what):
    """Check 1: assignment, similarity, counts, centroids and objective of one iteration from ``cent``."""
    xd, cd = dev(x), dev(cent)
    a2, sim = ops.backend().kmeans_assign(xd, cd)
    r, info, c = run_fit(xd, cd, 1)
    assert torch.equal(a2, r.assign), what
    N = x.shape[0]
    assert info == {"rows_valid": N, "rows_bad": 0, "iters_run": 1, "converged": 0, "empty": int((r.counts == 0).sum()), "unassigned": 0}
    assert r.changed.tolist() == [N]
    return cu.check_iteration(x, cent, sim_ref, r.assign.cpu().numpy(), sim.cpu().numpy(), r.counts.cpu().numpy(), c.cpu().numpy(),
                              float(r.objective[0]), what)


# ---- 1. one iteration, teacher-forced ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cu.STEP_CASES, ids=str)
def test_one_iteration_matches_fp64_reference(case):
    cu.assert_step_conditions(case)
    x, _, cent = cu.step_inputs(case)
    one_iteration(x, cent, cu.step_reference(case)[0], f"step {case}")


# ---- 2. equality with the search -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(129, 5, 34), (257, 129, 200), (65, 300, 30)], ids=str)
def test_assignment_is_the_search_with_one_neighbour(case):
    """assign and sim against rsp_cosine_topk(k = 1), bit for bit (its distance is clip(1 - s, 0, 2) in fp32), with a planted exact
    tie -- two identical centroids, the lower index wins -- and a zero centroid (similarity exactly 0, returnable)."""
    N, C, D = case
    x, _, cent = cu.step_inputs(case)
    cent = np.array(cent)
    hi = C - 1
    cent[1] = x[0]                      # row 0's own direction ...
    cent[hi] = cent[1]                  # ... twice: clusters 1 and C - 1 tie exactly on every row
    cent[2] = 0
    be = ops.backend()
    xd, cd = dev(x), dev(cent)
    a, sim = be.kmeans_assign(xd, cd)
    idx, dist = be.cosine_topk(xd, cd, 1)
    assert torch.equal(a, idx[:, 0])
    assert torch.equal(bits((1.0 - sim).clamp(0.0, 2.0)), bits(dist[:, 0]))
    idx2, dist2 = be.cosine_topk(xd, cd, 2)       # the general insertion path: its first entry is the k = 1 specialisation's only one
    assert torch.equal(a, idx2[:, 0]) and torch.equal(bits(dist[:, 0]), bits(dist2[:, 0]))
    assert int(a[0]) == 1 and not bool((a == hi).any()) and bool((a == 1).any())
    assert bool((sim[a == 2] == 0).all())
    # a zero centroid against one other: it takes exactly the rows whose similarity to the other is negative
    two = np.stack([np.zeros(D, dtype=np.float32), cent[3]])
    a, sim = be.kmeans_assign(xd, dev(two))
    ref = cluster.reference_similarities(x, two)[:, 1]
    clear = np.abs(ref) > cu.SIM_TOL
    assert np.array_equal((a.cpu().numpy() == 0)[clear], (ref < 0)[clear]) and bool((sim[a == 0] == 0).all())


def test_one_neighbour_specialisation_equals_the_general_search():
    """The search's k = 1 instance (the wave's arg-max of a tile) against its general instance (k = 2, first entry), bit for bit, over
    several gallery tiles and splits, with exact ties inside a tile, across tiles and across splits, a zero row and a NaN row."""
    q, _ = feats(41, 130, 34, 10, 0.5)
    g, _ = feats(42, 3000, 34, 10, 0.5)
    g = np.array(g)
    g[11] = g[10]               # inside a tile
    g[700] = g[10]              # another tile
    g[2990] = g[10]             # another split
    g[2991] = q[0]
    g[5] = q[0]
    g[100] = 0
    g[101, 3] = np.nan
    be = ops.backend()
    qd, gd = dev(q), dev(g)
    assert ops.backend().lib.rsp_cosine_topk_splits(130, 3000, 0) > 1
    for splits in (0, 1, 24):
        i1, d1 = be.cosine_topk(qd, gd, 1, splits=splits)
        i2, d2 = be.cosine_topk(qd, gd, 2, splits=splits)
        assert torch.equal(i1[:, 0], i2[:, 0]) and torch.equal(bits(d1[:, 0]), bits(d2[:, 0])), splits
    assert int(i1[0, 0]) == 5 and not bool(torch.isin(i1, torch.tensor([11, 700, 2990, 2991, 101], device=DEV)).any())


# ---- 3. whole fits, exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cu.EXACT_FITS, ids=str)
def test_whole_fit_reproduces_the_reference_exactly(case):
    cu.assert_exact_conditions(case)
    x, _, init = cu.exact_inputs(case)
    ref = cu.exact_reference(case)
    xd = dev(x)
    iters = case[5] + 4
    r, info, c = run_fit(xd, init, iters)
    assert info == ref.info and info["converged"] == 1 and info["iters_run"] == case[5]
    assert np.array_equal(r.changed.cpu().numpy(), ref.changed)
    assert np.array_equal(r.assign.cpu().numpy(), ref.assign) and np.array_equal(r.counts.cpu().numpy(), ref.counts)
    cu.check_trace_tail(r.changed.cpu().numpy(), r.objective.cpu().numpy(), case[5])
    err = float(np.abs(r.objective.cpu().numpy()[:case[5]] - ref.objective[:case[5]]).max())
    print(f"exact {case}: objective error {err:.3g}")
    assert err <= cu.SIM_TOL
    # the assignment of every iteration: the fit cut short after t + 1 iterations
    for t in range(case[5]):
        rt, it, _ = run_fit(xd, init, t + 1)
        assert np.array_equal(rt.assign.cpu().numpy(), ref.assigns[t]), t
        assert it["iters_run"] == t + 1 and it["converged"] == (1 if t + 1 == case[5] else 0)


# ---- 4. whole fits, teacher-forced per iteration ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cu.FORCED_FITS, ids=str)
def test_every_iteration_from_the_reference_centroids(case):
    cu.assert_forced_conditions(case)
    x, _, _ = cu.forced_inputs(case)
    ref = cu.forced_reference(case)
    for t in range(ref.info["iters_run"]):
        one_iteration(x, ref.cents[t], cluster.reference_similarities(x, ref.cents[t]), f"forced {case} t={t}")


# ---- 5. empty clusters ---------------------------------------------------------------------------------------------------------
def test_empty_clusters_keep_their_centroids():
    x, _, cent = cu.empty_inputs()
    N, D, C = cu.EMPTY_CASE
    r, info, c = run_fit(dev(x), cent, 1)
    assert info["empty"] == 324 and info["unassigned"] == 0
    counts = r.counts.cpu().numpy()
    assert (counts[N:] == 0).all() and int(counts.sum()) == N
    empty = counts == 0
    assert np.array_equal(c.cpu().numpy()[empty].view(np.int32), cent[empty].view(np.int32))
    cu.check_iteration(x, cent, cluster.reference_similarities(x, cent), r.assign.cpu().numpy(), None, counts, c.cpu().numpy(),
                       float(r.objective[0]), "empty clusters")


# ---- 6. non-finite values and invalid rows ---------------------------------------------------------------------------------------
def test_invalid_rows_take_part_in_nothing():
    """Zero rows, rows with a NaN and rows with an Inf (255 and 256: the last lane of one 256-row trip of the compaction and the first of
    the next): assign -1, counted in rows_bad, and every output of the fit is, to the bit,
    that of the fit on x without them."""
    x, _ = feats(3, 300, 34, 5, 1.0)
    x = np.array(x)
    bad = [0, 63, 64, 255, 256, 299]
    x[0] = 0
    x[63, 33] = np.nan
    x[64, 0] = np.inf
    x[255, 1] = np.nan
    x[256] = 0
    x[299, 7] = -np.inf
    init = x[[5, 50, 100, 150, 200]].copy()
    got, gi, gc = run_fit(dev(x), init, 30)
    want, wi, wc = run_fit(dev(np.delete(x, bad, axis=0)), init, 30)
    assert gi["rows_bad"] == 6 and gi["rows_valid"] == 294 and wi["rows_bad"] == 0
    assert {k: v for k, v in gi.items() if k != "rows_bad"} == {k: v for k, v in wi.items() if k != "rows_bad"}
    assert got.assign[bad].tolist() == [-1] * 6
    keep = np.delete(np.arange(300), bad)
    assert torch.equal(got.assign[keep], want.assign) and torch.equal(got.counts, want.counts) and torch.equal(got.changed, want.changed)
    assert torch.equal(bits(gc), bits(wc)) and torch.equal(bits(got.objective), bits(want.objective))
    ref = cluster.kmeans_reference(x, init, 30)
    assert gi["rows_valid"] == ref.info["rows_valid"] and gi["unassigned"] == 0
    a, sim = ops.backend().kmeans_assign(dev(x), gc)
    assert a[bad].tolist() == [-1] * 6 and bool(torch.isnan(sim[bad]).all()) and torch.equal(a, got.assign)


def test_a_nan_centroid_is_never_assigned():
    x, _ = feats(3, 300, 34, 5, 1.0)
    init = np.array(x[[5, 50, 100, 150, 200]])
    init[1, 3] = np.nan
    init[4, 0] = np.inf
    r, info, c = run_fit(dev(x), init, 2)
    a = r.assign.cpu().numpy()
    assert not np.isin(a, [1, 4]).any() and (a >= 0).all() and info["unassigned"] == 0 and info["empty"] == 2
    assert r.counts[[1, 4]].tolist() == [0, 0]
    assert np.array_equal(c.cpu().numpy()[[1, 4]].view(np.int32), init[[1, 4]].view(np.int32))
    r1, _, c1 = run_fit(dev(x), init, 1)
    cu.check_iteration(x, init, cluster.reference_similarities(x, init), r1.assign.cpu().numpy(), None, r1.counts.cpu().numpy(),
                       c1.cpu().numpy(), float(r1.objective[0]), "nan centroid")
    # nothing returnable: every valid row is unassigned, nothing moves, the fit stops at t = 1
    allnan = np.full((5, 34), np.nan, dtype=np.float32)
    r, info, c = run_fit(dev(x), allnan, 4)
    assert info == {"rows_valid": 300, "rows_bad": 0, "iters_run": 2, "converged": 1, "empty": 5, "unassigned": 300}
    assert bool((r.assign == -1).all()) and r.changed.tolist() == [300, 0, -1, -1] and r.counts.tolist() == [0] * 5
    assert r.objective[:2].tolist() == [0.0, 0.0] and bool(torch.isnan(r.objective[2:]).all()) and bool(torch.isnan(c).all())


# ---- 7. determinism and capture ----------------------------------------------------------------------------------------------
def _outputs(r, c):
    return [c, r.assign, r.counts, r.changed, r.objective, r.info]


def _same(a, b):
    return all(torch.equal(bits(p) if p.dtype != torch.uint8 else p, bits(q) if q.dtype != torch.uint8 else q) for p, q in zip(a, b))


@pytest.mark.parametrize("which", ["converging", "not converging"])
def test_same_bits_over_runs_and_under_capture(which):
    """Three eager runs, then the whole fit captured as one graph and replayed twice.  The converging case stops at iteration 6 of 12:
    the launches behind the stop are no-ops, eagerly and replayed."""
    if which == "converging":
        x, _, init = cu.exact_inputs(cu.EXACT_FITS[0])
        iters = 12
    else:
        x, _, init = cu.forced_inputs(cu.FORCED_FITS[1])
        iters = 4
    xd, i0 = dev(x), dev(init)
    r, info, c = run_fit(xd, i0, iters)
    assert info["converged"] == (1 if which == "converging" else 0)
    eager = _outputs(r, c)
    for _ in range(2):
        r2, _, c2 = run_fit(xd, i0, iters)
        assert _same(eager, _outputs(r2, c2))
    cap_c = i0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = ops.backend().kmeans_fit(xd, cap_c, iters)
    cap = _outputs(rc, cap_c)
    for _ in range(2):
        cap_c.copy_(i0)
        for t_ in cap[1:]:
            t_.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager, cap)


# ---- 8. guarded memory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(129, 34, 7, 3, 0), (300, 70, 130, 2, 1)], ids=str)
def test_guarded_memory(case):
    """Every operand, output and the workspace inside 0xFF-filled allocations at the alignment the header promises: x (row pitch D + 2,
    the gap is NaN), cent and the workspace on 8 bytes and not 16.  No byte outside them changes, x does not change, every element
    of every output is written (max_iters = the iterations the fit runs -- the second case converges in its last one --: no output
    element is legitimately -1 or NaN), and the gap's NaNs reach no output.  Then the same for the assign call and the contingency table."""
    N, D, C, iters, converged = case
    x, y = feats(21, N, D, C, 0.5)
    init = x[np.random.default_rng(4).choice(N, C, replace=False)].copy()
    ref = cluster.kmeans_reference(x, init, iters)
    assert ref.info["converged"] == converged and ref.info["iters_run"] == iters
    assert min(float(g.min()) for g in ref.gaps) > 10 * cu.SIM_GAP      # the trajectory's length does not hang on a near tie
    be = ops.backend()
    with Guarded(DEV, skew=8) as G:
        wide = G.alloc((N, D + 2), name="wide x")
        wide[:, :D] = dev(x)
        xd = wide[:, :D]
        before = wide.clone()
        cent = G.alloc((C, D), name="cent")
        cent.copy_(dev(init))
        yd = G.put(torch.from_numpy(np.array(y)))
        assert xd.data_ptr() % 16 == 8 and cent.data_ptr() % 16 == 8 and xd.stride(0) == D + 2
        r = be.kmeans_fit(xd, cent, iters)
        G.check()
        kinds = sorted(blk.kind for blk in G.blocks)
        assert kinds == ["input", "operand", "operand"] + ["output"] * 5 + ["workspace"], kinds
        assert torch.equal(bits(wide), bits(before)) and bool((wide.view(torch.int32)[:, D:] == -1).all())
        info = cluster.read_info(r.info)
        assert {k: info[k] for k in ("rows_valid", "rows_bad", "iters_run", "converged", "unassigned")} == \
            {"rows_valid": N, "rows_bad": 0, "iters_run": iters, "converged": converged, "unassigned": 0}
        a, counts, changed, obj = r.assign.cpu().numpy(), r.counts.cpu().numpy(), r.changed.cpu().numpy(), r.objective.cpu().numpy()
        assert (a >= 0).all() and (counts >= 0).all() and counts.sum() == N and (changed >= 0).all() and np.isfinite(obj).all()
        got_cent = cent.cpu().numpy()
        assert np.isfinite(got_cent).all()
        a2, sim = be.kmeans_assign(xd, cent)
        table, dropped = be.contingency(r.assign, yd, C, C)
        G.check()
        assert torch.equal(bits(wide), bits(before))
        assert bool(torch.isfinite(sim).all()) and bool((a2 >= 0).all())
        want = np.zeros((C, C), dtype=np.int64)
        np.add.at(want, (a, y), 1)
        assert np.array_equal(table.cpu().numpy(), want) and int(dropped) == 0
    # the last update is the sum over the returned assignment
    sums = cluster.update_reference(x, a, ref.cents[-1])
    full = counts > 0
    assert np.allclose(got_cent[full], sums[full], rtol=0, atol=2 * (counts.max() + 4) * 2.0 ** -24 * counts.max())
    assert np.array_equal(counts, np.bincount(a, minlength=C))


# ---- 9. contingency ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5, 1024])
def test_contingency_is_exact(L):
    rng = np.random.default_rng(L)
    N, C = 5000, 37
    a = rng.integers(-1, C, N).astype(np.int32)
    y = rng.integers(-2, L + 2, N).astype(np.int64)
    table, dropped = ops.backend().contingency(dev(a), dev(y), C, L)
    keep = (a >= 0) & (y >= 0) & (y < L)
    want = np.zeros((C, L), dtype=np.int64)
    np.add.at(want, (a[keep], y[keep]), 1)
    assert np.array_equal(table.cpu().numpy(), want) and int(dropped) == int((~keep).sum()) and int(dropped) > 0
    full, none = ops.backend().contingency(dev(np.abs(a)), dev(np.clip(y, 0, L - 1)), C, L)
    assert int(full.sum()) == N and int(none) == 0
    one, _ = ops.backend().contingency(dev(np.zeros(1, dtype=np.int32)), dev(np.zeros(1, dtype=np.int64)), 1024, L)
    assert int(one[0, 0]) == 1 and int(one.sum()) == 1


# ---- 10. bad arguments and a workspace one byte short ------------------------------------------------------------------------------
def test_bad_arguments_and_a_short_workspace_launch_nothing():
    N, D, C, iters = 129, 34, 7, 3
    x, y = feats(21, N, D, C, 0.5)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with Guarded(DEV, skew=8) as G:
        xd = G.put(torch.from_numpy(x))
        cent = G.put(torch.from_numpy(x[:C].copy()))
        yd = G.put(torch.from_numpy(y))
        assign, counts, changed = G.alloc((N,), torch.int32), G.alloc((C,), torch.int32), G.alloc((iters,), torch.int32)
        obj, info, sim = G.alloc((iters,), torch.float64), G.alloc((32,), torch.uint8), G.alloc((N,), torch.float32)
        table, dropped = G.alloc((C, C), torch.int64), G.alloc((1,), torch.int64)
        need = lib.rsp_kmeans_workspace(N, D, C)
        ws = G.alloc((need,), torch.uint8)

        def fit(N_=N, D_=D, C_=C, iters_=iters, wsb=need):
            return lib.rsp_kmeans_fit(p(xd), D, N_, D_, p(cent), C_, iters_, p(assign), p(counts), p(changed), p(obj), p(info), p(ws), wsb, None)
        assert fit(wsb=need - 1) == -2 and lib.rsp_last_error() == b"rsp_kmeans_fit: workspace too small"
        for kw in (dict(N_=0), dict(D_=33), dict(C_=0), dict(C_=1025), dict(iters_=0), dict(iters_=1001)):
            assert fit(**kw) == -1 and lib.rsp_last_error().startswith(b"rsp_kmeans_fit: "), kw
        need_a = lib.rsp_cosine_topk_workspace(N, C, D, 1, 0)
        assert lib.rsp_kmeans_assign(p(xd), D, N, D, p(cent), C, p(assign), p(sim), p(ws), need_a - 1, None) == -2
        assert lib.rsp_kmeans_assign(p(xd), D, N, D, p(cent), 0, p(assign), p(sim), p(ws), need, None) == -1
        assert lib.rsp_last_error().startswith(b"rsp_kmeans_assign: ")
        assert lib.rsp_contingency(p(assign), p(yd), N, C, 0, p(table), p(dropped), None) == -1
        assert lib.rsp_contingency(p(assign), p(yd), N, 1025, C, p(table), p(dropped), None) == -1
        assert lib.rsp_last_error().startswith(b"rsp_contingency: ")
        G.check()                          # bands intact, the three inputs unchanged
        for out in (assign, counts, changed, obj, info, sim, table, dropped, ws):
            assert bool((out.view(torch.uint8) == FILL).all())


# ---- 11. the monitor -------------------------------------------------------------------------------------------------------------
def test_monitor_run_leaves_the_model_and_the_generators_alone():
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory
    torch.manual_seed(3)
    model = ModelFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=DEV)
    net = model.module
    net.train()
    net.encoder_k.eval()                                   # a mixed set of flags: every module gets its own back
    mon = cluster.ClusterMonitor(every=1, num_epochs=1, num_clusters=3, num_classes=3, bank_samples=24, batch_size=4, max_iters=20)
    (bank,) = mon.build_loaders(16, 32, DEV, seed=0)
    before = {n: t_.clone() for n, t_ in net.state_dict().items()}
    flags = [m.training for m in net.modules()]
    states = (random.getstate(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(DEV).clone())
    out = mon.run(model, bank)
    assert set(out) == {"nmi", "ari", "purity", "objective", "iters", "empty", "n_bank", "bad_rows", "seconds"}
    assert out["n_bank"] == 24 and out["bad_rows"] == 0 and 1 <= out["iters"] <= 20 and 0 <= out["empty"] < 3
    assert 0 <= out["nmi"] <= 1 + 1e-12 and -1 <= out["ari"] <= 1 and 1 / 3 <= out["purity"] <= 1 and -1 <= out["objective"] <= 1 + 1e-6
    after = net.state_dict()
    assert list(after) == list(before)
    for n, t_ in after.items():
        assert torch.equal(t_, before[n]), n
    assert [m.training for m in net.modules()] == flags
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    assert torch.equal(torch.cuda.get_rng_state(DEV), states[2])
    again = mon.run(model, bank)
    assert all(again[k] == out[k] for k in out if k != "seconds")
    mon_k = cluster.ClusterMonitor(every=1, num_epochs=1, num_clusters=4, num_classes=3, encoder="k", bank_samples=24, batch_size=4,
                                   max_iters=5, restarts=2)
    assert 0 <= mon_k.run(model, bank)["purity"] <= 1


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
    """Two epochs, the monitor every second one: its scalars are in the second line only.  Without the key no line carries such a
    scalar and the backend's kmeans_fit is never called; both runs train the same model, line for line and checkpoint for checkpoint."""
    from rspnet_amd.pretrain import main_worker
    be = ops.backend()
    calls = []
    inner = be.kmeans_fit

    def counted(x, *a, **kw):
        calls.append(tuple(x.shape))
        return inner(x, *a, **kw)
    be.kmeans_fit = counted
    try:
        keys = {"cluster_monitor": {"every": 2, "num_clusters": 3, "num_classes": 3, "bank_samples": 24, "batch_size": 4, "max_iters": 20}}
        main_worker(0, _args(tmp_path, keys, "with"), "")
        with_calls = list(calls)
        del calls[:]
        main_worker(0, _args(tmp_path, {}, "without"), "")
        without_calls = list(calls)
    finally:
        del be.kmeans_fit
    lines = {name: [json.loads(l) for l in open(tmp_path / name / "exp" / "run_0_t" / "scalars.jsonl")] for name in ("with", "without")}
    assert len(lines["with"]) == 2 and len(lines["without"]) == 2
    first, second = lines["with"]
    assert not any(k.startswith("cluster_") for k in first)
    assert sorted(k for k in second if k.startswith("cluster_")) == ["cluster_ari", "cluster_empty", "cluster_iters", "cluster_nmi",
                                                                     "cluster_objective", "cluster_purity"]
    assert all(np.isfinite(second[k]) for k in second if k.startswith("cluster_"))
    assert len(with_calls) == 1 and with_calls[0][0] == 24 and without_calls == []
    assert not any(k.startswith("cluster_") for rec in lines["without"] for k in rec)
    for a, b in zip(lines["with"], lines["without"]):
        assert {k: v for k, v in a.items() if not k.startswith("cluster_")} == b      # the loss trajectory is bit-identical
    a = torch.load(tmp_path / "with" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    b = torch.load(tmp_path / "without" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n
