"""CPU: the label-free representation statistics -- the definitions on known cases, the torch composition against the fp64
restatement (rspnet_amd.repr_stats.repr_reference), the Gram identity, invalid rows, the entry point's argument checks on dummy
pointers, the monitor's configuration and schedule, and the command-line tool."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

from cpu_ops import CpuOps
from repr_util import case_input, case_reference, check
from rspnet_amd import _lib, ops, repr_stats

SHAPES = [(2, 2), (65, 30), (129, 34), (300, 70), (1000, 128)]


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())      # has no repr_stats: repr_stats.raw_stats composes the rule from torch ops
    yield
    ops.set_backend(prev)


def test_definitions_on_isotropic_and_collapsed_rows():
    """N = 1000 standard normal rows in D = 128: s is close to N(0, 1 / D), so the mean of exp(4 (s - 1)) is exp(-4 + 8 / D) and the
    uniformity -3.9375 (-3.938 measured with the restatement); nearly full rank (125.9 measured).  Rows 1 + 1e-3 noise: every cosine
    is 1 - O(1e-6), one singular value carries everything (uniformity -4.1e-6, effective rank 1.11 measured at N = 200, D = 128)."""
    iso = repr_stats.summarize(case_reference(1000, 128))
    print(iso)
    assert iso["effective_rank"] > 120 and abs(iso["uniformity"] + 3.9375) < 0.01
    assert abs(iso["mean_cos"]) < 1e-3 and abs(iso["mean_cos2"] - 1 / 128) < 1e-3
    assert 0.9 < iso["dim_std_min"] <= iso["dim_std_mean"] < 1.01 and (iso["rows"], iso["bad_rows"]) == (1000, 0)
    col = repr_stats.summarize(case_reference(200, 128, "collapsed"))
    print(col)
    assert -1e-3 < col["uniformity"] <= 0 and col["effective_rank"] < 1.5
    assert col["mean_cos"] > 0.999 and col["dim_std_mean"] < 0.01


@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_torch_composition_matches_reference(shape, kind, cpu_backend):
    got = repr_stats.raw_stats(torch.from_numpy(case_input(*shape, kind).copy()), 2.0)
    check(got, case_reference(*shape, kind), f"torch composition {shape} {kind}")


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gram_identity(shape):
    """||gram||_F^2 = sum_ij s_ij^2 = M + 2 pair_cos2: the two halves of the reference agree with each other."""
    r = case_reference(*shape)
    lhs, rhs = float((r["gram"] ** 2).sum()), r["rows_valid"] + 2.0 * r["pair_cos2"]
    print(shape, lhs, rhs, abs(lhs - rhs) / rhs)
    assert abs(lhs - rhs) <= 1e-6 * rhs


def planted_invalid(N=130, D=34):
    x = np.array(case_input(N, D))
    x[3] = 0
    x[64, 5] = np.nan
    x[129, 33] = np.inf
    return x, np.delete(x, [3, 64, 129], axis=0)


def test_invalid_rows_take_part_in_nothing(cpu_backend):
    x, kept = planted_invalid()
    ref_full, ref_kept = repr_stats.repr_reference(x), repr_stats.repr_reference(kept)
    assert (ref_full["rows_valid"], ref_full["rows_bad"]) == (127, 3) and ref_kept["rows_bad"] == 0
    for k in ("pair_exp", "pair_cos", "pair_cos2"):
        assert ref_full[k] == ref_kept[k], k
    assert np.array_equal(ref_full["gram"], ref_kept["gram"]) and np.array_equal(ref_full["colsum"], ref_kept["colsum"])
    got = repr_stats.raw_stats(torch.from_numpy(x), 2.0)
    check(dict(got, rows_bad=0), ref_kept, "torch composition, three invalid rows")
    out = repr_stats.repr_stats(torch.from_numpy(x))
    want = repr_stats.summarize(ref_kept)
    assert out["bad_rows"] == 3 and out["rows"] == 127
    for k in ("uniformity", "mean_cos", "mean_cos2", "effective_rank", "dim_std_min", "dim_std_mean"):
        assert out[k] == pytest.approx(want[k], rel=1e-4, abs=1e-6), k


def test_fewer_than_two_valid_rows(cpu_backend):
    x = np.zeros((3, 4), dtype=np.float32)
    x[1] = [1, 2, 3, 4]
    x[2, 0] = np.nan
    for out in (repr_stats.summarize(repr_stats.repr_reference(x)), repr_stats.repr_stats(torch.from_numpy(x))):
        assert math.isnan(out["uniformity"]) and math.isnan(out["mean_cos"]) and math.isnan(out["mean_cos2"])
        assert (out["rows"], out["bad_rows"]) == (1, 2)
        assert out["effective_rank"] == pytest.approx(1.0, abs=1e-5) and out["dim_std_min"] == 0
    none = repr_stats.summarize(repr_stats.repr_reference(np.zeros((2, 4), dtype=np.float32)))
    assert all(math.isnan(none[k]) for k in ("uniformity", "effective_rank", "dim_std_min")) and none["rows"] == 0
    for bad in (0.0, -1.0, 32.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            repr_stats.repr_stats(torch.from_numpy(x), t=bad)


def test_argument_checks_of_the_entry_point():
    """RSP_EINVAL / RSP_EWORKSPACE with the entry point's name, on dummy pointers: nothing is dereferenced, nothing is launched."""
    lib = _lib.load()
    P, ODD = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    need = lib.rsp_repr_stats_workspace(300, 64)

    def call(x=P, ld=64, N=300, D=64, c=4.0, sums=P, gram=P, colsum=P, ws=P, wsb=1 << 30):
        return lib.rsp_repr_stats(x, ld, N, D, c, sums, gram, colsum, ws, wsb, None)
    for kw, what in ((dict(D=63), b"bad size"), (dict(ld=62), b"bad size"), (dict(ld=65), b"bad size"), (dict(N=0), b"bad size"),
                     (dict(N=262145), b"bad size"), (dict(D=4098, ld=4098), b"bad size"), (dict(D=0), b"bad size"),
                     (dict(c=0.0), b"c must be finite and in (0, 64]"), (dict(c=float("nan")), b"c must be finite and in (0, 64]"),
                     (dict(c=64.5), b"c must be finite and in (0, 64]"), (dict(c=float("inf")), b"c must be finite and in (0, 64]"),
                     (dict(c=-1.0), b"c must be finite and in (0, 64]"), (dict(colsum=None), b"gram and colsum go together"),
                     (dict(gram=None), b"gram and colsum go together"), (dict(x=ODD), b"8-byte aligned"),
                     (dict(sums=None), b"null pointer"), (dict(x=None), b"null pointer")):
        assert call(**kw) == -1, kw
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_repr_stats: ") and what in err, (kw, err)
    assert need > 0 and call(wsb=need - 1) == -2 and lib.rsp_last_error() == b"rsp_repr_stats: workspace too small"
    assert call(wsb=need - 1, gram=None, colsum=None) == -2
    sizes = [lib.rsp_repr_stats_workspace(N, 128) for N in (1, 2, 63, 64, 65, 128, 129, 300, 4096, 16384, 16385, 100000, 262144)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    dense = [lib.rsp_repr_stats_workspace(N, 34) for N in range(1, 2000)]
    assert dense == sorted(dense)
    assert lib.rsp_repr_stats_workspace(0, 128) == 0 and lib.rsp_repr_stats_workspace(8, 3) == 0
    assert ctypes.sizeof(_lib.ReprSums) == 40 and lib.rsp_version() == 130


def test_monitor_from_config_and_schedule():
    assert repr_stats.ReprMonitor.from_config({}, 10) is None
    assert repr_stats.ReprMonitor.from_config({"repr_monitor": {"every": 0, "t": 2.0}}, 10) is None
    m = repr_stats.ReprMonitor.from_config({"repr_monitor": {"every": 3, "t": 3.0}}, 10)
    assert (m.every, m.t, m.num_epochs) == (3, 3.0, 10)
    assert [e for e in range(10) if m.due(e)] == [2, 5, 8, 9]      # every third epoch, and the last
    d = repr_stats.ReprMonitor.from_config({"repr_monitor": {"every": 1}}, 2)
    assert d.t == 2.0 and d.due(0) and d.due(1)
    for bad in ({"t": 0}, {"t": 33}, {"t": float("nan")}, {"k": 5}, {"no_such_key": 1}):
        with pytest.raises(ValueError):
            repr_stats.ReprMonitor.from_config({"repr_monitor": dict({"every": 1}, **bad)}, 10)


def test_pretext_configs_do_not_carry_the_key():
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = glob.glob(os.path.join(root, "rspnet_amd", "config", "pretrain", "*.json"))
    assert paths and all("repr_monitor" not in json.load(open(p)) for p in paths)


def test_monitor_reads_the_queue_and_refuses_a_capture(cpu_backend, monkeypatch):
    net = torch.nn.Module()
    net.register_buffer("queue", torch.nn.functional.normalize(torch.from_numpy(case_input(300, 70).copy()).t(), dim=0))
    before, state = net.queue.clone(), torch.get_rng_state().clone()
    out = repr_stats.ReprMonitor(every=1, num_epochs=1).run(net)
    want = repr_stats.summarize(case_reference(300, 70))
    assert out["rows"] == 300 and out["uniformity"] == pytest.approx(want["uniformity"], abs=1e-5)
    assert out["effective_rank"] == pytest.approx(want["effective_rank"], rel=1e-4) and "seconds" in out
    assert torch.equal(net.queue, before) and torch.equal(torch.get_rng_state(), state)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        repr_stats.ReprMonitor(every=1, num_epochs=1).run(net)


def test_knn_monitor_hands_back_the_bank_features_only_when_asked():
    import inspect
    from rspnet_amd import knn
    assert inspect.signature(knn.KNNMonitor.run).parameters["return_features"].default is False


def test_command_line_tool(cpu_backend, tmp_path, caplog):
    train, test = case_input(300, 70), case_input(129, 34)
    for split, X in (("train", train), ("test", np.pad(test, ((0, 0), (0, 36))))):
        np.save(tmp_path / f"{split}_fold2_feats.npy", X.astype(np.float64))
        np.save(tmp_path / f"{split}_fold2_labels.npy", np.zeros(len(X), dtype=np.int64))
    with caplog.at_level("INFO", logger="rspnet_amd.repr_stats"):
        out = repr_stats.main(["--features", str(tmp_path), "--fold", "2", "--t", "2.0"])
    with open(tmp_path / "repr_fold2.json") as f:
        saved = json.load(f)
    assert saved == out and set(saved) == {"uniformity", "mean_cos", "mean_cos2", "effective_rank", "dim_std_min", "dim_std_mean",
                                           "rows", "bad_rows", "t"}
    want = repr_stats.summarize(case_reference(300, 70))
    assert saved["t"] == 2.0 and (saved["rows"], saved["bad_rows"]) == (300, 0)
    for k in ("uniformity", "mean_cos", "effective_rank", "dim_std_min"):
        assert saved[k] == pytest.approx(want[k], rel=1e-4, abs=1e-6), k
    assert f"Repr train fold 2 t=2.0: uniformity {saved['uniformity']:.4f}" in caplog.text and "300 rows (0 bad)" in caplog.text
    # --max-rows 100 keeps every ceil(300 / 100) = 3rd row; --split test reads the other file
    sub = repr_stats.main(["--features", str(tmp_path), "--fold", "2", "--max-rows", "100"])
    assert sub["rows"] == 100
    assert sub["uniformity"] == pytest.approx(repr_stats.summarize(repr_stats.repr_reference(train[::3]))["uniformity"], abs=1e-5)
    assert repr_stats.main(["--features", str(tmp_path), "--fold", "2", "--max-rows", "250"])["rows"] == 150      # ceil(300 / 250) = 2
    assert repr_stats.main(["--features", str(tmp_path), "--fold", "2", "--split", "test"])["rows"] == 129
