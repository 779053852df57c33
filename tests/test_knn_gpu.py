"""GPU: rsp_knn_classify (HipOps.knn_classify) against the fp64 definition, against the retrieval search, on planted ties, over
runs and split counts, under capture; the monitor alone and inside the pretext driver."""
import ctypes
import json
import random
import types

import numpy as np
import pytest
import torch

from knn_util import CAP, CASES, case_inputs, case_reference, check_votes, excused
from rspnet_amd import _lib, knn, ops
from test_retrieval_gpu import check_against_fp64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(*arrays):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in arrays]      # (a copy: the shared inputs are read-only)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def own_hits(res, valid):
    r = res.rank[:valid]
    return [int((r < 1).sum()), int((r < 5).sum())]


def ref_pred(votes):
    return votes.argmax(axis=1)          # numpy: the first maximum, i.e. the lower class


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_knn_matches_fp64_reference(case):
    Nq, Ng, D, C, k, T, a = case
    q, yq, g, yg = case_inputs(case)
    rank, votes, idx, sim, nxt, exc = case_reference(case)
    print(f"{case}: {int(exc.sum())} of {Nq} queries excused")
    assert exc.sum() <= CAP * Nq
    tq, tyq, tg, tyg = dev(q, yq, g, yg)
    res = ops.backend().knn_classify(tq, tg, tyg, k, T, C, y_q=tyq, want_idx=True, want_votes=True)
    keep = ~exc
    assert np.array_equal(res.rank.cpu().numpy()[keep], rank[keep])
    assert np.array_equal(res.pred.cpu().numpy()[keep], ref_pred(votes)[keep])
    worst = check_votes(res.votes.cpu().numpy(), votes, keep)
    print(f"  worst vote error {worst:.2e} of the largest vote")
    assert res.hits.cpu().tolist() == own_hits(res, Nq)
    swapped, total = check_against_fp64(q, g, k, res.idx, res.dist)
    assert swapped <= 0.5 * total


def planted_search_inputs(Nq, Ng, D, copies_of_row_5):
    rng = np.random.default_rng(14)
    q = rng.standard_normal((Nq, D)).astype(np.float32)
    g = rng.standard_normal((Ng, D)).astype(np.float32)
    if copies_of_row_5:
        g[list(copies_of_row_5)] = g[5]
        q[0], q[1] = g[5], 2.0 * g[5]                       # two queries whose best neighbours are the tied rows
    return q, g, rng.integers(0, 4, Ng)


# k alone: the seeded case 5.  (Nq, Ng, D, k, splits, copies of gallery row 5): the two places where the callers of the one S = 1 search
# could still differ -- Ng < k (the tail is -1 / +inf through both stores, D off the 32-wide chunk), and ties that straddle the tile
# boundary (rows 127 | 128) and the boundary of the two splits, merged by both callers.
@pytest.mark.parametrize("k, planted", [pytest.param(1, None, id="1"), pytest.param(20, None, id="20"), pytest.param(64, None, id="64"),
                                        pytest.param(64, (9, 40, 66, 0, ()), id="short_gallery"),
                                        pytest.param(20, (70, 300, 130, 2, (127, 128, 200)), id="ties_on_tile_and_split_boundary")])
def test_neighbours_equal_the_retrieval_search_bit_for_bit(k, planted):
    if planted is None:
        case, splits = CASES[5], 0
        q, yq, g, yg = dev(*case_inputs(case))
        C = case[3]
    else:
        Nq, Ng, D, splits, copies = planted
        q, g, yg = dev(*planted_search_inputs(Nq, Ng, D, copies))
        C = 4
    be = ops.backend()
    idx, dist = be.cosine_topk(q, g, k, splits=splits)
    res = be.knn_classify(q, g, yg, k, 0.07, C, want_idx=True, splits=splits)
    assert res.rank is None and res.hits is None and res.votes is None
    assert torch.equal(res.idx, idx) and torch.equal(bits(res.dist), bits(dist))
    if planted is not None:
        row = res.idx[0].cpu().tolist()
        if copies:
            assert row[:4] == [5, 127, 128, 200] and res.idx[1].cpu().tolist()[:4] == row[:4]      # the ties, lower index first
        else:
            assert sorted(row[:Ng]) == list(range(Ng)) and row[Ng:] == [-1] * (k - Ng) and bool(torch.isinf(res.dist[0, Ng:]).all())


@pytest.mark.parametrize("k", [3, 200])
def test_tie_straddling_rank_k_goes_to_the_lower_index(k):
    rng = np.random.default_rng(11)
    g = rng.standard_normal((900, 64)).astype(np.float32)
    dups = np.sort(rng.choice(900, k + 60, replace=False))
    g[dups] = g[dups[0]]                                   # k + 60 identical rows: the query's best, all at one similarity
    q = np.stack([g[dups[0]], 2.0 * g[dups[0]]])
    yg = rng.integers(0, 4, 900)
    tq, tg, tyg = dev(q, g, yg)
    res = ops.backend().knn_classify(tq, tg, tyg, k, 0.07, 4, want_idx=True, splits=3)
    for row in res.idx.cpu().numpy():
        assert row.tolist() == dups[:k].tolist()           # the k lowest indices are in, in order; the higher ones are out


def test_equal_weight_sequences_tie_to_the_lower_class():
    """Every gallery row exists twice, rows 2i and 2i + 1, the first labelled 3 and the second 1: the neighbour list is pair after pair
    (a tie goes to the lower index), so with an even k the classes 3 and 1 receive the same weights in the same order."""
    rng = np.random.default_rng(12)
    half = rng.standard_normal((200, 64)).astype(np.float32)
    g = np.repeat(half, 2, axis=0)
    yg = np.tile(np.array([3, 1]), 200)
    q = rng.standard_normal((10, 64)).astype(np.float32)
    yq = np.array([1, 3] * 5)
    tq, tyq, tg, tyg = dev(q, yq, g, yg)
    res = ops.backend().knn_classify(tq, tg, tyg, 200, 0.07, 5, y_q=tyq, want_idx=True, want_votes=True)
    idx, votes = res.idx.cpu().numpy(), res.votes.cpu()
    assert np.array_equal(idx[:, 0::2] + 1, idx[:, 1::2]) and np.all(idx[:, 0::2] % 2 == 0)
    assert torch.equal(bits(votes[:, 3]), bits(votes[:, 1])) and bool((votes[:, 1] > 0).all())
    assert bool((votes[:, [0, 2, 4]] == 0).all())
    assert res.pred.cpu().tolist() == [1] * 10
    assert res.rank.cpu().tolist() == [0, 1] * 5           # target 1 wins the tie, target 3 is behind class 1
    assert res.hits.cpu().tolist() == [5, 10]


def test_zero_rows_bad_labels_and_valid():
    rng = np.random.default_rng(13)
    Nq, Ng, D, C, k, T = 40, 700, 64, 7, 100, 0.1
    q, g = rng.standard_normal((Nq, D)).astype(np.float32), rng.standard_normal((Ng, D)).astype(np.float32)
    yq, yg = rng.integers(0, C, Nq), rng.integers(0, C, Ng)
    q[3] = 0
    g[[0, 50, 699]] = 0
    yg[[1, 2, 60]] = [-1, C, 1 << 40]                      # cast no vote
    yq[[5, 6]] = [-1, C]                                   # misses
    rank, votes, idx, sim, nxt = knn.knn_reference(q, yq, g, yg, k, T, C)
    exc = excused(yq, votes, sim, nxt, k)
    tq, tyq, tg, tyg = dev(q, yq, g, yg)
    for valid in (None, 17, 0):
        res = ops.backend().knn_classify(tq, tg, tyg, k, T, C, y_q=tyq, valid=valid, want_idx=True, want_votes=True)
        got = res.rank.cpu().numpy()
        assert np.array_equal(got[~exc], rank[~exc]) and got[5] == C and got[6] == C
        check_votes(res.votes.cpu().numpy(), votes, ~exc)
        assert res.hits.cpu().tolist() == own_hits(res, Nq if valid is None else valid)
    # the zero query: similarity 0 to everything, so its neighbours are rows 0 .. k-1 at distance 1, each with weight exp(-1 / T)
    assert res.idx[3].cpu().tolist() == list(range(k)) and bool((res.dist[3] == 1).all())
    w = np.float32(np.exp(np.float32(-1.0) * np.float32(1.0 / np.float32(T))))
    counts = np.bincount(yg[:k][(yg[:k] >= 0) & (yg[:k] < C)], minlength=C)
    assert np.allclose(res.votes[3].cpu().numpy(), counts * w, rtol=1e-5)
    check_against_fp64(q, g, k, res.idx, res.dist)


def test_deterministic_across_runs_and_splits():
    lib = ops.backend().lib
    rng = np.random.default_rng(14)
    q = torch.from_numpy(rng.standard_normal((300, 512)).astype(np.float32)).to(DEV)
    g = torch.from_numpy((rng.standard_normal((20000, 512)) + 0.5 * rng.standard_normal((1, 512))).astype(np.float32)).to(DEV)
    g[1000:1010] = g[10]                                   # ties: copies of row 10 in its own split ...
    g[12000:12005] = g[10]                                 # ... and across split boundaries (3, 7 and the automatic 19 splits)
    g[19990:20000] = g[6000]                               # a second group, its copies in the last tile
    q[:20] = g[10] + 0.01 * q[:20]                         # queries whose lists hold the tied rows
    q[20:40] = g[6000] + 0.01 * q[20:40]
    yg = torch.from_numpy(rng.integers(0, 101, 20000)).to(DEV)
    yq = torch.from_numpy(rng.integers(0, 101, 300)).to(DEV)
    used = {lib.rsp_cosine_topk_splits(300, 20000, s) for s in (0, 1, 3, 7)}
    assert len(used) >= 3
    be = ops.backend()
    ref = be.knn_classify(q, g, yg, 200, 0.07, 101, y_q=yq, want_idx=True, want_votes=True)
    planted = ref.idx[:20].cpu().numpy()
    assert all(row[:16].tolist() == [10] + list(range(1000, 1010)) + list(range(12000, 12005)) for row in planted)
    for s in (0, 1, 3, 7):
        for _ in range(2):
            res = be.knn_classify(q, g, yg, 200, 0.07, 101, y_q=yq, want_idx=True, want_votes=True, splits=s)
            assert torch.equal(res.idx, ref.idx) and torch.equal(bits(res.dist), bits(ref.dist)), s
            assert torch.equal(bits(res.votes), bits(ref.votes)) and torch.equal(res.rank, ref.rank), s
            assert torch.equal(res.pred, ref.pred) and torch.equal(res.hits, ref.hits), s


def test_no_nq_by_ng_allocation():
    Nq, Ng, D = 4096, 65536, 512
    q = torch.randn(Nq, D, device=DEV)
    g = torch.randn(Ng, D, device=DEV)
    yg = torch.randint(0, 400, (Ng,), device=DEV)
    yq = torch.randint(0, 400, (Nq,), device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    res = ops.backend().knn_classify(q, g, yg, 200, 0.07, 400, y_q=yq)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak growth {grown / 2**20:.1f} MiB vs {Nq * Ng * 4 / 2**20:.0f} MiB for the matrix")
    assert grown < Nq * Ng * 4
    assert res.pred.shape == (Nq,) and res.hits.cpu().tolist() == own_hits(res, Nq)


def test_bad_arguments_are_rejected_before_any_launch():
    be = ops.backend()
    q, g = torch.randn(8, 64, device=DEV), torch.randn(50, 64, device=DEV)
    yg, yq = torch.zeros(50, dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    call = lambda k=5, T=0.07, C=3, q=q, g=g: be.knn_classify(q, g, yg, k, T, C, y_q=yq)
    for kw, what in ((dict(k=0), "k must be in [1, 256]"), (dict(k=257), "k must be in [1, 256]"),
                     (dict(C=1025), "num_classes must be in [1, 1024]"), (dict(C=0), "num_classes must be in [1, 1024]"),
                     (dict(T=0.001), "T must be finite and >= 0.01"), (dict(T=float("nan")), "T must be finite and >= 0.01"),
                     (dict(T=float("inf")), "T must be finite and >= 0.01"),
                     (dict(q=torch.randn(8, 63, device=DEV), g=torch.randn(50, 63, device=DEV)), "bad size")):
        with pytest.raises(_lib.RspError) as e:
            call(**kw)
        assert "rsp_knn_classify: " in str(e.value) and what in str(e.value), str(e.value)
    # through the C entry point itself, on dummy pointers (nothing is dereferenced): rank and y_q go together, hits needs y_q,
    # valid in [0, Nq], the workspace size
    lib = be.lib
    P = ctypes.c_void_p(1 << 20)
    raw = lambda yq, rank, hits, valid=8, wsb=1 << 30: lib.rsp_knn_classify(P, 64, 8, yq, P, 64, 50, P, 64, 5, 0.07, 3, 0, valid, None,
                                                                           None, None, P, rank, hits, P, wsb, None)
    for args, rc, what in (((None, P, None), -1, b"rank is required with y_q and only with it"),
                           ((P, None, None), -1, b"rank is required with y_q and only with it"),
                           ((None, None, P), -1, b"hits needs y_q"), ((P, P, P, 9), -1, b"valid must be in [0, Nq]"),
                           ((P, P, P, -1), -1, b"valid must be in [0, Nq]"), ((P, P, P, 8, 16), -2, b"workspace too small")):
        assert raw(*args) == rc, args
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_knn_classify: ") and what in err, err
    assert call().pred.shape == (8,)


def test_capture_and_replay_give_the_same_bits():
    case = CASES[3]
    Nq, Ng, D, C, k, T, a = case
    q, yq, g, yg = dev(*case_inputs(case))
    be = ops.backend()
    eager = be.knn_classify(q, g, yg, k, T, C, y_q=yq, want_idx=True, want_votes=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = be.knn_classify(q, g, yg, k, T, C, y_q=yq, want_idx=True, want_votes=True)
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a_, b_ in zip(cap, eager):
            assert torch.equal(bits(a_), bits(b_))


# ---- the monitor ---------------------------------------------------------------------------------------------------------
def test_monitor_run_leaves_the_model_and_the_generators_alone():
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory
    torch.manual_seed(3)
    model = ModelFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=DEV)
    net = model.module
    net.train()
    net.encoder_k.eval()                                   # a mixed set of flags: every module gets its own back
    mon = knn.KNNMonitor(every=1, num_epochs=1, k=8, t=0.07, num_classes=3, bank_samples=24, query_samples=12, batch_size=4)
    bank, query = mon.build_loaders(16, 32, DEV, seed=0)
    before = {n: t.clone() for n, t in net.state_dict().items()}
    flags = [m.training for m in net.modules()]
    states = (random.getstate(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(DEV).clone())
    out = mon.run(model, bank, query)
    assert set(out) == {"acc1", "acc5", "n_bank", "n_query", "seconds"}
    assert out["n_bank"] == 24 and out["n_query"] == 12 and 0 <= out["acc1"] <= out["acc5"] <= 100
    after = net.state_dict()
    assert list(after) == list(before)
    for n, t in after.items():
        assert torch.equal(t, before[n]), n
    assert [m.training for m in net.modules()] == flags
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    assert torch.equal(torch.cuda.get_rng_state(DEV), states[2])
    # the key encoder, and the same features twice: the same answer
    mon_k = knn.KNNMonitor(every=1, num_epochs=1, k=8, num_classes=3, encoder="k", bank_samples=24, query_samples=12, batch_size=4)
    again = mon.run(model, bank, query)
    assert (again["acc1"], again["acc5"]) == (out["acc1"], out["acc5"])
    assert 0 <= mon_k.run(model, bank, query)["acc1"] <= 100


def _args(tmp_path, knn_key, name):
    cfg = json.load(open("rspnet_amd/config/pretrain/c3d.json"))
    cfg.update(batch_size=4, num_epochs="2", log_interval=2)
    cfg["moco"]["k"] = 64
    cfg["spatial_transforms"]["size"] = 32
    if knn_key is not None:
        cfg["knn_monitor"] = knn_key
    (tmp_path / name).mkdir()
    p = tmp_path / name / "cfg.json"
    json.dump(cfg, open(p, "w"))
    exp = tmp_path / name / "exp"
    return types.SimpleNamespace(config=str(p), ext_config=None, experiment_dir=str(exp), load_checkpoint=None, load_model=None,
                                 debug=False, world_size=1, seed=0, no_scale_lr=False, steps_per_epoch=3, run_dir=str(exp / "run_0_t"),
                                 cont=False)


def test_pretext_driver_with_and_without_the_monitor(tmp_path):
    """The monitor's scalars appear with the key and only with it, and the run with the monitor trains exactly what the run
    without it trains: checkpoint for checkpoint."""
    from rspnet_amd.pretrain import main_worker
    key = {"every": 1, "k": 8, "num_classes": 3, "bank_samples": 24, "query_samples": 12, "batch_size": 4}
    main_worker(0, _args(tmp_path, key, "with"), "")
    main_worker(0, _args(tmp_path, None, "without"), "")
    lines = {name: [json.loads(l) for l in open(tmp_path / name / "exp" / "run_0_t" / "scalars.jsonl")] for name in ("with", "without")}
    assert len(lines["with"]) == 2 and len(lines["without"]) == 2
    for rec in lines["with"]:
        for name in ("knn/acc1", "knn/acc5"):
            assert np.isfinite(rec[name]) and 0 <= rec[name] <= 100
    assert not any(k.startswith("knn/") for rec in lines["without"] for k in rec)
    a = torch.load(tmp_path / "with" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    b = torch.load(tmp_path / "without" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n
