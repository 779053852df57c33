"""The pretext driver's monitor loop without a device: Engine._run_monitors / Engine._write_scalars on a stand-in engine for each of the
five monitor classes, with ``run`` replaced by a recorder (the driver itself binds to the device; its end-to-end runs are GPU tests),
the kNN -> repr hand-off of the bank features, and the one from_config of the base class."""
import json
import os
import types

import pytest
import torch

from rspnet_amd import repr_stats
from rspnet_amd.cluster import ClusterMonitor
from rspnet_amd.knn import KNNMonitor
from rspnet_amd.linear_probe import LinearProbeMonitor
from rspnet_amd.pretrain import MONITORS, Engine
from rspnet_amd.repr_stats import ReprMonitor
from rspnet_amd.tsne import TsneMonitor

STATS = {k: {"avg": float(i)} for i, k in enumerate(("loss", "loss_A", "acc1_A", "acc5_A", "loss_M", "acc1_M"))}
MODEL = types.SimpleNamespace(module=types.SimpleNamespace(queue=torch.zeros(16, 8)))
REPR_RESULT = {"uniformity": -1.5, "mean_cos": 0.125, "mean_cos2": 0.25, "effective_rank": 5.5, "dim_std_min": 0.0625, "dim_std_mean": 0.5,
               "rows": 8, "bad_rows": 1, "seconds": 0.1}

# class, constructor arguments, loaders, what run returns, the arguments run must get behind the model ({run_dir}: the directory of
# scalars.jsonl), the scalars of the epoch's line, the log line
CASES = [
    (KNNMonitor, dict(k=20, t=0.07), ("bank", "query"), {"acc1": 50.0, "acc5": 75.0, "n_bank": 24, "n_query": 12, "seconds": 0.1},
     ("bank", "query"), {"knn/acc1": 50.0, "knn/acc5": 75.0},
     "kNN [1/2]\tAcc@1 50.00\tAcc@5 75.00\t(k=20, T=0.07, bank 24, query 12, 0.1 s)"),
    (ReprMonitor, dict(t=2.0), (), REPR_RESULT, (),
     {"repr/uniformity": -1.5, "repr/mean_cos": 0.125, "repr/effective_rank": 5.5, "repr/dim_std_min": 0.0625, "repr/bad_rows": 1},
     "Repr [1/2]\tuniformity -1.5000\teff.rank 5.5/16\tmean cos 0.1250\tdim std min 0.062\t(t=2.0, 8 rows, 1 bad, 0.10 s)"),
    (LinearProbeMonitor, dict(steps=20, lr=0.125), ("bank", "query"),
     {"acc1": 50.0, "acc5": 75.0, "loss": 1.25, "train_loss": 0.5, "n_bank": 24, "n_query": 12, "bad_rows": 0, "seconds": 0.1},
     ("bank", "query"), {"probe_acc1": 50.0, "probe_acc5": 75.0, "probe_loss": 1.25},
     "Probe [1/2]\tAcc@1 50.00\tAcc@5 75.00\tloss 1.2500\t(20 steps, lr 0.125, bank 24, query 12, 0 bad, 0.1 s)"),
    (ClusterMonitor, dict(num_clusters=5), ("bank",),
     {"nmi": 0.5, "ari": 0.25, "purity": 0.75, "objective": 0.9, "iters": 7, "empty": 1, "n_bank": 24, "bad_rows": 0, "seconds": 0.1},
     ("bank",), {"cluster_nmi": 0.5, "cluster_ari": 0.25, "cluster_purity": 0.75, "cluster_objective": 0.9, "cluster_iters": 7,
                 "cluster_empty": 1},
     "Cluster [1/2]\tNMI 0.5000\tARI 0.2500\tpurity 0.7500\tobjective 0.9000\t(5 clusters, 7 iterations, 1 empty, bank 24, 0 bad, 0.1 s)"),
    (TsneMonitor, dict(perplexity=30, iters=500), ("bank",), {"kl": 1.5, "purity": 0.75, "n_bank": 24, "bad_rows": 0, "seconds": 0.1},
     ("bank", os.path.join("{run_dir}", "tsne_epoch1")), {"tsne_kl": 1.5, "tsne_purity": 0.75},
     "t-SNE [1/2]\tKL 1.5000\tpurity@10 0.7500\t(perplexity 30, 500 iterations, bank 24, 0 bad, 0.1 s)"),
]


def stand_in(monitors, loaders, path, rank=0, num_epochs=2):
    return types.SimpleNamespace(monitors=monitors, monitor_loaders=loaders if rank == 0 else {}, monitor_results={}, local_rank=rank,
                                 current_epoch=0, num_epochs=num_epochs, model=MODEL, stats=STATS, scalars_path=path)


def run_epochs(e, num_epochs):
    for epoch in range(num_epochs):
        e.current_epoch = epoch
        Engine._run_monitors(e)
        Engine._write_scalars(e, 0.05)
    return [json.loads(line) for line in open(e.scalars_path)]


def test_the_list_is_the_five_monitors_in_their_order():
    assert MONITORS == tuple(c[0] for c in CASES)
    assert [cls.KEY for cls in MONITORS] == ["knn_monitor", "repr_monitor", "probe_monitor", "cluster_monitor", "tsne_monitor"]


@pytest.mark.parametrize("cls,kw,loaders,result,args,scalars,line", CASES, ids=[c[0].__name__ for c in CASES])
def test_pretext_driver_wiring_without_a_device(tmp_path, caplog, cls, kw, loaders, result, args, scalars, line):
    """The monitor runs when due and only then, with exactly the expected arguments, on rank 0 only; its scalars -- the exact key set
    and values -- go into that epoch's line and into no other, every other number of every line is what it is without the monitor, and
    its log line has the driver's wording."""
    calls = []

    def make():
        mon = cls(every=2, num_epochs=2, **kw)      # due after epoch 1 only
        mon.run = lambda *a, **k: calls.append((a, k)) or dict(result)
        return mon

    with caplog.at_level("INFO", logger="rspnet_amd.pretrain"):
        with_ = run_epochs(stand_in([make()], {cls.KEY: loaders}, tmp_path / "with.jsonl"), 2)
    without = run_epochs(stand_in([], {}, tmp_path / "without.jsonl"), 2)
    assert calls == [((MODEL,) + tuple(a.format(run_dir=str(tmp_path)) for a in args), {})]
    assert not set(scalars) & set(without[1])
    assert with_[0] == without[0] and with_[1] == {**without[1], **scalars}
    assert [r.getMessage() for r in caplog.records] == [line]
    other = stand_in([make()], {cls.KEY: loaders}, None, rank=1)
    other.current_epoch = 1
    Engine._run_monitors(other)
    assert other.monitor_results == {} and len(calls) == 1


def test_knn_hands_the_bank_features_to_repr_only_when_both_are_due(tmp_path, monkeypatch):
    """return_features is requested only in an epoch in which repr_monitor is due as well, repr/bank_* is in exactly those lines, and
    features never stay behind for a later epoch."""
    bank = torch.ones(6, 4)
    knn_calls, bank_calls = [], []

    def knn_run(model, *loaders, **k):
        knn_calls.append(k)
        out = {"acc1": 50.0, "acc5": 75.0, "n_bank": 6, "n_query": 3, "seconds": 0.1}
        return dict(out, bank_features=bank) if k.get("return_features") else out

    def bank_stats(x, t):
        bank_calls.append((x, t))
        return {"uniformity": -2.5, "effective_rank": 3.5, "dim_std_min": 0.25, "mean_cos": 0.0, "rows": 6, "bad_rows": 0}

    monkeypatch.setattr(repr_stats, "repr_stats", bank_stats)
    knn, rep = KNNMonitor(every=2, num_epochs=6), ReprMonitor(every=3, num_epochs=6, t=1.5)      # due after 1, 3, 5 / after 2, 5
    knn.run, rep.run = knn_run, lambda model: dict(REPR_RESULT)
    e = stand_in([knn, rep], {knn.KEY: ("bank", "query"), rep.KEY: ()}, tmp_path / "s.jsonl", num_epochs=6)
    lines = run_epochs(e, 6)
    assert knn_calls == [{}, {}, {"return_features": True}]
    assert len(bank_calls) == 1 and bank_calls[0][0] is bank and bank_calls[0][1] == 1.5
    assert "bank_features" not in e.monitor_results[knn.KEY]
    assert ["knn/acc1" in rec for rec in lines] == [False, True, False, True, False, True]
    assert ["repr/uniformity" in rec for rec in lines] == [False, False, True, False, False, True]
    bank_keys = {"repr/bank_uniformity": -2.5, "repr/bank_effective_rank": 3.5, "repr/bank_dim_std_min": 0.25}
    for epoch, rec in enumerate(lines):
        assert {k: v for k, v in rec.items() if k.startswith("repr/bank_")} == (bank_keys if epoch == 5 else {})


@pytest.mark.parametrize("cls", MONITORS, ids=[cls.__name__ for cls in MONITORS])
def test_from_config_looks_at_the_keys_of_an_enabled_block_only(cls):
    assert cls.KEYS[0] == "every"
    assert cls.from_config({cls.KEY: {"every": 0, "no_such_key": 1}}, 10) is None
    with pytest.raises(ValueError, match=f"{cls.KEY}: unknown keys"):
        cls.from_config({cls.KEY: {"every": 1, "no_such_key": 1}}, 10)
    m = cls.from_config({cls.KEY: {"every": 4}}, 10)
    assert isinstance(m, cls) and [ep for ep in range(10) if m.due(ep)] == [3, 7, 9]
