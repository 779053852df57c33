"""CPU: the weighted kNN classifier's definition (rspnet_amd.knn.knn_reference) on a hand-made case, its torch composition against
that definition on the seeded cases, the monitor's configuration and schedule, and the command-line tool."""
import json
import math

import numpy as np
import pytest
import torch

from cpu_ops import CpuOps
from knn_util import CAP, CASES, case_inputs, case_reference, check_votes
from rspnet_amd import knn, ops


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())      # has no knn_classify: knn.knn_classify composes the rule from torch ops
    yield
    ops.set_backend(prev)


# 2-D features, 6 gallery rows, 3 classes, k = 4, T = 0.5: w = exp((s - 1) / 0.5) = exp(2 s - 2)
HAND_G = np.array([[1, 0], [0.8, 0.6], [0.6, 0.8], [0, 1], [-1, 0], [0.6, -0.8]], dtype=np.float32)
HAND_YG = np.array([0, 1, 1, 2, 2, 0])
HAND_Q = np.array([[1, 0], [0, 3]], dtype=np.float32)      # (the second: a row of norm 3, direction (0, 1))
HAND_YQ = np.array([1, 2])


def test_reference_on_a_hand_made_case():
    rank, votes, idx, sim, nxt = knn.knn_reference(HAND_Q, HAND_YQ, HAND_G, HAND_YG, 4, 0.5, 3)
    e = math.exp
    # query 0 = (1, 0): s = 1, .8, .6, 0, -1, .6 -> neighbours 0 (1), 1 (.8), then the tie at .6: row 2 before row 5; row 3 (0) is next
    assert idx[0].tolist() == [0, 1, 2, 5]
    assert np.allclose(sim[0], [1, 0.8, 0.6, 0.6], atol=1e-7) and abs(nxt[0]) < 1e-7
    #   class 0: rows 0 and 5: 1 + e(-.8); class 1: rows 1 and 2: e(-.4) + e(-.8); class 2: nothing
    assert np.allclose(votes[0], [1 + e(-0.8), e(-0.4) + e(-0.8), 0], rtol=1e-6)
    assert rank[0] == 1                                       # target 1: class 0 has more
    # query 1 = (0, 3): s = 0, .6, .8, 1, 0, -.8 -> neighbours 3 (1), 2 (.8), 1 (.6), then the tie at 0: row 0 before row 4
    assert idx[1].tolist() == [3, 2, 1, 0]
    #   class 0: row 0 (s = 0): e(-2); class 1: rows 2 (.8) and 1 (.6): e(-.4) + e(-.8); class 2: row 3 (1): 1
    assert np.allclose(votes[1], [e(-2), e(-0.4) + e(-0.8), 1], rtol=1e-6)
    assert rank[1] == 1                                       # target 2 (vote 1) is behind class 1 (1.1196)


def test_reference_edges():
    # Ng < k: only Ng neighbours vote, the tail is -1 / -inf, and there is no (k+1)-th
    rank, votes, idx, sim, nxt = knn.knn_reference(HAND_Q, HAND_YQ, HAND_G[:3], HAND_YG[:3], 4, 0.5, 3)
    assert idx[0].tolist() == [0, 1, 2, -1] and np.isinf(sim[0, 3]) and np.isinf(nxt).all()
    # a gallery label outside [0, C) casts no vote; a query label outside is a miss (rank = C); a zero row has similarity 0
    yg = HAND_YG.copy()
    yg[0] = 7
    q = np.array([[1, 0], [0, 0]], dtype=np.float32)
    rank, votes, idx, sim, nxt = knn.knn_reference(q, np.array([-1, 0]), HAND_G, yg, 4, 0.5, 3)
    assert votes[0, 0] == pytest.approx(math.exp(-0.8)) and rank[0] == 3
    assert idx[1].tolist() == [0, 1, 2, 3] and np.all(sim[1] == 0)
    # equal votes: the tie goes to the lower class (target 1 ties with class 0 -> rank 1; target 0 -> rank 0)
    g2 = np.array([[1, 0], [1, 0]], dtype=np.float32)
    for t, want in ((1, 1), (0, 0)):
        rank = knn.knn_reference(q[:1], np.array([t]), g2, np.array([0, 1]), 2, 0.07, 2)[0]
        assert rank[0] == want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:5]))
def test_torch_composition_matches_reference(case, cpu_backend):
    Nq, Ng, D, C, k, T, a = case
    q, yq, g, yg = case_inputs(case)
    rank, votes, idx, sim, nxt, exc = case_reference(case)
    print(f"{case}: {int(exc.sum())} of {Nq} queries excused")
    assert exc.sum() <= CAP * Nq
    tq, tyq, tg, tyg = (torch.from_numpy(x.copy()) for x in (q, yq, g, yg))
    res = knn.knn_classify(tq, tyq, tg, tyg, k=k, T=T, num_classes=C)
    keep = ~exc
    assert np.array_equal(res["rank"].numpy()[keep], rank[keep])
    assert res["n"] == Nq and res["hits"] == (int((res["rank"] < 1).sum()), int((res["rank"] < 5).sum()))
    assert res["acc1"] == pytest.approx(100.0 * res["hits"][0] / Nq)
    _, _, tvotes = knn._knn_torch(tq, tyq, tg, tyg, k, T, C)
    worst = check_votes(tvotes.numpy(), votes, keep)
    print(f"  worst vote error {worst:.2e} of the largest vote")


def test_valid_cuts_the_tail(cpu_backend):
    case = CASES[3]
    q, yq, g, yg = (torch.from_numpy(x.copy()) for x in case_inputs(case))
    full = knn.knn_classify(q, yq, g, yg, k=case[4], T=case[5], num_classes=case[3])
    cut = knn.knn_classify(q, yq, g, yg, k=case[4], T=case[5], num_classes=case[3], valid=100)
    assert cut["n"] == 100 and cut["hits"] == (int((full["rank"][:100] < 1).sum()), int((full["rank"][:100] < 5).sum()))
    with pytest.raises(ValueError):
        knn.knn_classify(q, yq, g, yg, k=case[4], T=case[5], num_classes=case[3], valid=131)


def test_monitor_from_config_and_schedule():
    assert knn.KNNMonitor.from_config({}, 10) is None
    assert knn.KNNMonitor.from_config({"knn_monitor": {"every": 0, "k": 8}}, 10) is None
    m = knn.KNNMonitor.from_config({"knn_monitor": {"every": 3, "k": 8, "t": 0.1, "num_classes": 3, "encoder": "k", "bank_samples": 24,
                                                    "query_samples": 12, "batch_size": 4, "n_crop": 2}}, 10)
    assert (m.every, m.k, m.t, m.num_classes, m.encoder, m.bank_samples, m.query_samples, m.batch_size, m.n_crop) == \
        (3, 8, 0.1, 3, "k", 24, 12, 4, 2)
    assert [e for e in range(10) if m.due(e)] == [2, 5, 8, 9]      # every third epoch, and the last
    d = knn.KNNMonitor.from_config({"knn_monitor": {"every": 1}}, 2)
    assert (d.k, d.t, d.num_classes, d.encoder) == (200, 0.07, 101, "q") and d.due(0) and d.due(1)
    for bad in ({"k": 0}, {"k": 257}, {"t": 0.001}, {"t": float("nan")}, {"t": float("inf")}, {"num_classes": 0}, {"num_classes": 1025},
                {"encoder": "v"}, {"bank_samples": 0}, {"no_such_key": 1}):
        with pytest.raises(ValueError):
            knn.KNNMonitor.from_config({"knn_monitor": dict({"every": 1}, **bad)}, 10)


def test_pretext_configs_do_not_carry_the_key():
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = glob.glob(os.path.join(root, "rspnet_amd", "config", "pretrain", "*.json"))
    assert paths and all("knn_monitor" not in json.load(open(p)) for p in paths)


def test_command_line_tool(cpu_backend, tmp_path, caplog):
    case = CASES[3]
    Nq, Ng, D, C, k, T, a = case
    q, yq, g, yg = case_inputs(case)
    for split, X, y in (("train", g, yg), ("test", q, yq)):
        np.save(tmp_path / f"{split}_fold2_feats.npy", X.astype(np.float64))
        np.save(tmp_path / f"{split}_fold2_labels.npy", y)
    with caplog.at_level("INFO", logger="rspnet_amd.knn"):
        out = knn.main(["--features", str(tmp_path), "--fold", "2", "--k", "200", "--t", "0.07"])
    nc = int(max(yq.max(), yg.max())) + 1
    rank, votes, idx, sim, nxt = knn.knn_reference(q, yq, g, yg, 200, 0.07, nc)
    with open(tmp_path / "knn_fold2.json") as f:
        saved = json.load(f)
    assert saved == out and set(saved) == {"k", "t", "acc1", "acc5", "hits1", "hits5", "total"}
    assert case_reference(case)[5].sum() == 0                  # no query of this case is excused: the counts are the reference's
    assert (saved["hits1"], saved["hits5"], saved["total"]) == (int((rank < 1).sum()), int((rank < 5).sum()), Nq)
    assert saved["k"] == 200 and saved["t"] == 0.07 and saved["acc1"] == pytest.approx(100.0 * saved["hits1"] / Nq)
    line = f"kNN k=200 T=0.07: Acc@1 = {saved['acc1']:.2f}% ({saved['hits1']}/{Nq}), Acc@5 = {saved['acc5']:.2f}% ({saved['hits5']}/{Nq})"
    assert line in caplog.text


def test_monitor_refuses_to_run_inside_a_capture(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        knn.KNNMonitor(every=1, num_epochs=1).run(None, [], [])


def test_argument_checks_of_the_entry_point():
    """RSP_EINVAL / RSP_EWORKSPACE with the entry point's name, on dummy pointers: nothing is dereferenced, nothing is launched."""
    import ctypes
    from rspnet_amd import _lib
    lib = _lib.load()
    P, ODD = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    def call(q=P, ldq=64, yq=P, D=64, k=5, T=0.07, C=3, valid=8, rank=P, hits=P, wsb=1 << 30, idx=None, dist=None):
        return lib.rsp_knn_classify(q, ldq, 8, yq, P, 64, 50, P, D, k, T, C, 0, valid, idx, dist, None, P, rank, hits, P, wsb, None)
    for kw, what in ((dict(k=0), b"k must be in [1, 256]"), (dict(k=257), b"k must be in [1, 256]"),
                     (dict(C=0), b"num_classes must be in [1, 1024]"), (dict(C=1025), b"num_classes must be in [1, 1024]"),
                     (dict(T=0.001), b"T must be finite"), (dict(T=float("nan")), b"T must be finite"), (dict(T=float("inf")), b"T must be finite"),
                     (dict(D=63), b"bad size"), (dict(ldq=63), b"bad size"), (dict(D=66), b"bad size"), (dict(q=ODD), b"8-byte aligned"),
                     (dict(yq=None), b"rank is required with y_q"), (dict(rank=None), b"rank is required with y_q"),
                     (dict(yq=None, rank=None), b"hits needs y_q"), (dict(valid=9), b"valid must be in [0, Nq]"),
                     (dict(valid=-1), b"valid must be in [0, Nq]"), (dict(idx=P), b"idx and dist go together")):
        assert call(**kw) == -1, kw
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_knn_classify: ") and what in err, (kw, err)
    need = lib.rsp_knn_classify_workspace(8, 50, 64, 5, 3, 0)
    assert need == lib.rsp_cosine_topk_workspace(8, 50, 64, 5, 0) > 0
    assert call(wsb=need - 1) == -2 and lib.rsp_last_error() == b"rsp_knn_classify: workspace too small"
