"""CPU: the linear probe's torch composition (linear_probe._probe_torch) against its definition (probe_reference) on the seeded
trajectories, the defaults on the full-batch cases, invalid rows, the limits, the monitor's configuration and the command-line tool."""
import ctypes
import json
import random

import numpy as np
import pytest
import torch

from cpu_ops import CpuOps
from probe_util import FULL_BATCH, TRAJECTORIES, case_inputs, check, hits, trajectory_reference
from rspnet_amd import _lib, linear_probe, ops


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())      # has no linear_probe_fit: linear_probe.fit_raw composes the rule from torch ops
    yield
    ops.set_backend(prev)


def _fit_from_zeros(x, y, C, batch, steps, **kw):
    """linear_probe.fit's defaults on the rows in their order (fit itself shuffles when batch < N)."""
    xt, yt = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))
    D = x.shape[1]
    w, b, mom = torch.zeros(C, D), torch.zeros(C), torch.zeros(C * D + C)
    lr = torch.from_numpy(linear_probe.lr_schedule(0.125, steps))
    trace, counts = linear_probe.fit_raw(xt, yt, w, b, mom, lr, steps, batch, **kw)
    return linear_probe.Probe(w, b, trace, counts, kw.get("normalize", True), kw.get("scale", 8.0))


@pytest.mark.parametrize("case", TRAJECTORIES, ids=str)
def test_torch_composition_matches_reference(case, cpu_backend):
    """fp32 torch ops against the fp64 rule over the whole trajectory at the suite's per-kernel gate; the predictions on the training
    rows are the reference's on every row (the fp64 top-two logit gap after the fit is at least 0.066 on these cases, some 1e3
    times the fp32 error of a logit)."""
    N, D, C, batch, steps = case
    x, y, _, _ = case_inputs(N, D, C)
    ref, zref = trajectory_reference(N, D, C, batch, steps)
    p = _fit_from_zeros(x, y, C, batch, steps)
    check(p.w.numpy(), p.b.numpy(), p.loss_trace.numpy(), ref, f"torch {case}")
    assert tuple(p.counts.tolist()) == ref.counts == (N, 0)
    z = linear_probe.logits(p, torch.from_numpy(np.array(x)))
    top2 = np.sort(zref, axis=1)[:, -2:]
    print(f"top-two gap {float((top2[:, 1] - top2[:, 0]).min()):.3f}")
    assert np.array_equal(z.argmax(dim=1).numpy(), zref.argmax(axis=1))


@pytest.mark.parametrize("shape", FULL_BATCH, ids=str)
def test_defaults_fit_the_clustered_inputs(shape):
    """The defaults, not the kernels: 100 full-batch steps of the fp64 rule reach training accuracy 1.0 with a loss that never rises."""
    N, D, C = shape
    ref, zref = trajectory_reference(N, D, C, N, 100)
    assert (zref.argmax(axis=1) == case_inputs(N, D, C)[1]).all()
    assert (np.diff(ref.loss_trace) <= 0).all() and ref.loss_trace[0] == pytest.approx(np.log(C))


def _with_invalid_rows(N, D, C):
    x, y, _, _ = case_inputs(N, D, C)
    x, y = np.array(x), np.array(y)
    bad = [0, 63, 64, 200, N - 1]
    x[0] = 0
    x[63, D - 1] = np.nan
    x[64, 0] = np.inf
    y[200] = -1
    y[N - 1] = C
    return x, y, bad


def test_invalid_rows_take_part_in_nothing(cpu_backend):
    """A zero row, a row with a NaN, a row with an Inf and the labels -1 and C: with batch = N the fit is, to the bit, the fit on the
    array without those rows; counts says how many there were."""
    N, D, C = 300, 34, 7
    x, y, bad = _with_invalid_rows(N, D, C)
    got = _fit_from_zeros(x, y, C, N, 100)
    want = _fit_from_zeros(np.delete(x, bad, axis=0), np.delete(y, bad), C, N - len(bad), 100)
    assert tuple(got.counts.tolist()) == (N - 5, 5) and tuple(want.counts.tolist()) == (N - 5, 0)
    for a, b in ((got.w, want.w), (got.b, want.b), (got.loss_trace, want.loss_trace)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ref = linear_probe.probe_reference(x, y, C, linear_probe.lr_schedule(0.125, 100), 100, N)
    assert ref.counts == (N - 5, 5)
    check(got.w.numpy(), got.b.numpy(), got.loss_trace.numpy(), ref, "five invalid rows")
    # the logits of an invalid row are NaN (the label plays no part there): a miss for evaluate
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    z = linear_probe.logits(got, xt)
    nan_rows = torch.isnan(z).any(dim=1).nonzero().reshape(-1).tolist()
    assert nan_rows == [0, 63, 64] and bool(torch.isnan(z[nan_rows]).all())
    res = linear_probe.evaluate(got, xt, yt)
    assert res["n"] == N and res["hits"][0] == N - 5 and set(res) == {"loss", "acc1", "acc5", "hits", "n", "pred", "rank"}
    assert res["rank"][[0, 63, 64, 200, N - 1]].tolist() == [C] * 5


def test_no_normalize_and_a_row_without_valid_rows(cpu_backend):
    N, D, C = 129, 30, 5
    x, y, _, _ = case_inputs(N, D, C)
    ref = linear_probe.probe_reference(x, y, C, linear_probe.lr_schedule(0.01, 20), 20, 64, normalize=False, scale=0.5)
    xt, yt = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))
    w, b, mom = torch.zeros(C, D), torch.zeros(C), torch.zeros(C * D + C)
    trace, counts = linear_probe.fit_raw(xt, yt, w, b, mom, torch.from_numpy(linear_probe.lr_schedule(0.01, 20)), 20, 64,
                                         normalize=False, scale=0.5)
    check(w.numpy(), b.numpy(), trace.numpy(), ref, "normalize = False")
    # every label out of range: m = 0 in every step, the loss is 0 and only the weight decay moves the state
    w0 = torch.full((C, D), 0.5)
    b0, mom0 = torch.full((C,), -0.25), torch.zeros(C * D + C)
    trace, counts = linear_probe.fit_raw(xt, torch.full_like(yt, C), w0, b0, mom0, torch.full((2,), 0.5), 2, N)
    assert trace.tolist() == [0.0, 0.0] and counts.tolist() == [0, N]
    ref = linear_probe.probe_reference(x, np.full(N, C), C, [0.5, 0.5], 2, N, w0=np.full((C, D), 0.5), b0=np.full(C, -0.25))
    assert np.allclose(w0.numpy(), ref.w, rtol=1e-6) and np.allclose(b0.numpy(), ref.b, rtol=1e-6)


def test_fit_shuffles_with_its_own_generator(cpu_backend):
    N, D, C = 129, 30, 5
    x, y, _, _ = case_inputs(N, D, C)
    xt, yt = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(y))
    states = (random.getstate(), torch.get_rng_state().clone())
    a = linear_probe.fit(xt, yt, C, steps=30, batch=64, seed=3)
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    b = linear_probe.fit(xt, yt, C, steps=30, batch=64, seed=3)
    c = linear_probe.fit(xt, yt, C, steps=30, batch=64, seed=4)
    assert torch.equal(a.w, b.w) and torch.equal(a.loss_trace, b.loss_trace) and not torch.equal(a.w, c.w)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).numpy()
    ref = linear_probe.probe_reference(x[perm], y[perm], C, linear_probe.lr_schedule(0.125, 30), 30, 64)
    check(a.w.numpy(), a.b.numpy(), a.loss_trace.numpy(), ref, "shuffled once")
    full = linear_probe.fit(xt, yt, C, steps=30)                   # full batch: the rows stay where they are
    ref = linear_probe.probe_reference(x, y, C, linear_probe.lr_schedule(0.125, 30), 30, N)
    check(full.w.numpy(), full.b.numpy(), full.loss_trace.numpy(), ref, "full batch")
    const = linear_probe.lr_schedule(0.25, 4, "constant")
    assert const.tolist() == [0.25] * 4 and linear_probe.lr_schedule(0.125, 100)[0] == np.float32(0.125)


def test_limits_raise_value_error(cpu_backend):
    x, y = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64)
    for kw in (dict(num_classes=0), dict(num_classes=1025), dict(batch=0), dict(batch=9), dict(steps=0)):
        args = dict(num_classes=3, steps=2, batch=None)
        args.update(kw)
        with pytest.raises(ValueError, match="linear_probe"):
            linear_probe.fit(x, y, **args)
    for bad in (torch.zeros(8, 3), torch.zeros(8, 4098), torch.zeros(0, 4)):
        with pytest.raises(ValueError, match="linear_probe"):
            linear_probe.fit(bad, torch.zeros(bad.shape[0], dtype=torch.int64), 3, steps=2)
    with pytest.raises(ValueError, match="schedule"):
        linear_probe.fit(x, y, 3, steps=2, schedule="step")
    with pytest.raises(ValueError, match="valid"):
        linear_probe.evaluate(linear_probe.fit(x + 1, y, 3, steps=1), x + 1, y, valid=9)


def test_argument_checks_of_the_entry_points():
    """RSP_EINVAL / RSP_EWORKSPACE with the entry point's name, on dummy pointers: nothing is dereferenced, nothing is launched."""
    lib = _lib.load()
    P, ODD = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)

    def fit(x=P, ld=64, N=100, D=64, y=P, C=7, batch=50, first=0, steps=3, w=P, counts=P, wsb=1 << 30):
        return lib.rsp_linear_probe_fit(x, ld, N, D, y, C, batch, first, steps, P, 0.9, 1e-4, 1, 8.0, w, P, P, P, counts, P, wsb, None)
    for kw, what in ((dict(C=0), b"bad size"), (dict(C=1025), b"bad size"), (dict(N=0), b"bad size"), (dict(D=63), b"bad size"),
                     (dict(D=4098, ld=4098), b"bad size"), (dict(ld=62), b"bad size"), (dict(ld=65), b"bad size"),
                     (dict(batch=0), b"bad step plan"), (dict(batch=101), b"bad step plan"), (dict(steps=0), b"bad step plan"),
                     (dict(first=-1), b"bad step plan"), (dict(x=ODD), b"8-byte aligned"), (dict(w=ODD), b"8-byte aligned"),
                     (dict(counts=None), b"null pointer"), (dict(y=None), b"null pointer")):
        assert fit(**kw) == -1, kw
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_linear_probe_fit: ") and what in err, (kw, err)
    need = lib.rsp_linear_probe_workspace(100, 64, 7, 50)
    assert need > 0 and fit(wsb=need - 1) == -2 and lib.rsp_last_error() == b"rsp_linear_probe_fit: workspace too small"
    for bad in ((0, 64, 7, 1), (100, 63, 7, 50), (100, 64, 0, 50), (100, 64, 1025, 50), (100, 64, 7, 0), (100, 64, 7, 101)):
        assert lib.rsp_linear_probe_workspace(*bad) == 0, bad

    def logits(x=P, ld=64, D=64, C=7, ld_out=7, out=P, wsb=1 << 30):
        return lib.rsp_linear_probe_logits(x, ld, 100, D, P, P, C, 1, 8.0, out, ld_out, P, wsb, None)
    for kw, what in ((dict(C=0), b"bad size"), (dict(D=66), b"bad size"), (dict(ld_out=6), b"bad size"), (dict(x=ODD), b"8-byte aligned"),
                     (dict(out=None), b"null pointer")):
        assert logits(**kw) == -1, kw
        err = lib.rsp_last_error()
        assert err.startswith(b"rsp_linear_probe_logits: ") and what in err, (kw, err)
    assert logits(wsb=100) == -2 and lib.rsp_version() == 130


def test_workspace_is_the_stated_formula():
    """f, the flags and the row lists (3 x 4 N), one int per chunk, G (batch x C), one loss partial per 64 rows, and the split
    partials of dW and db, each rounded up to 256 bytes.  splits = min(ceil(1024 / (ceil(C / 64) ceil(D / 128))), ceil(batch / 32)
    // 4), at least 1."""
    lib = _lib.load()
    up = lambda v: -(-v // 256) * 256
    for N, D, C, batch in ((9537, 512, 101, 9537), (300, 70, 300, 256), (129, 34, 7, 129), (16384, 2048, 400, 16384)):
        splits = max(1, min(-(-1024 // (-(-C // 64) * -(-D // 128))), -(-batch // 32) // 4))
        want = (3 * up(4 * N) + up(4 * -(-N // batch)) + up(4 * batch * C) + up(4 * -(-batch // 64)) + up(4 * splits * C * D)
                + up(4 * splits * C))
        assert lib.rsp_linear_probe_workspace(N, D, C, batch) == want, (N, D, C, batch)
    # at the UCF-101 fold: 74 splits; G is 3.9 MB and the partials 15.3 MB -- a small multiple of G plus the split partials
    g, parts = 4 * 9537 * 101, 4 * 74 * (101 * 512 + 101)
    assert g + parts <= lib.rsp_linear_probe_workspace(9537, 512, 101, 9537) <= 1.05 * (g + parts)


def test_monitor_from_config_and_schedule():
    assert linear_probe.LinearProbeMonitor.from_config({}, 10) is None
    assert linear_probe.LinearProbeMonitor.from_config({"probe_monitor": {"every": 0, "steps": 50}}, 10) is None
    m = linear_probe.LinearProbeMonitor.from_config({"probe_monitor": {"every": 4, "num_classes": 11, "steps": 50, "lr": 0.25,
                                                                      "momentum": 0.8, "weight_decay": 0.0, "scale": 4.0, "batch": 64,
                                                                      "encoder": "k", "bank_samples": 96, "query_samples": 32,
                                                                      "batch_size": 8, "n_crop": 2}}, 10)
    assert (m.every, m.num_classes, m.steps, m.lr, m.momentum, m.weight_decay, m.scale, m.batch, m.encoder) == \
        (4, 11, 50, 0.25, 0.8, 0.0, 4.0, 64, "k")
    assert (m.bank_samples, m.query_samples, m.batch_size, m.n_crop) == (96, 32, 8, 2)
    assert [e for e in range(10) if m.due(e)] == [3, 7, 9]
    with pytest.raises(ValueError, match="unknown keys"):
        linear_probe.LinearProbeMonitor.from_config({"probe_monitor": {"every": 1, "k": 5}}, 10)
    for kw in (dict(encoder="x"), dict(num_classes=0), dict(steps=0), dict(bank_samples=0), dict(batch=10 ** 6)):
        with pytest.raises(ValueError):
            linear_probe.LinearProbeMonitor(every=1, num_epochs=1, **kw)


def test_pretext_configs_do_not_carry_the_key():
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = glob.glob(os.path.join(root, "rspnet_amd", "config", "pretrain", "*.json"))
    assert paths and all("probe_monitor" not in json.load(open(p)) for p in paths)


def test_monitor_refuses_to_run_inside_a_capture(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        linear_probe.LinearProbeMonitor(every=1, num_epochs=1).run(None, [], [])


def test_command_line_tool(cpu_backend, tmp_path, caplog):
    N, D, C = 300, 34, 7
    x, y, x2, y2 = case_inputs(N, D, C, 120)
    for split, X, lab in (("train", x, y), ("test", x2, y2)):
        np.save(tmp_path / f"{split}_fold2_feats.npy", X.astype(np.float64))
        np.save(tmp_path / f"{split}_fold2_labels.npy", lab)
    with caplog.at_level("INFO", logger="rspnet_amd.linear_probe"):
        out = linear_probe.main(["--features", str(tmp_path), "--fold", "2", "--steps", "100"])
    with open(tmp_path / "probe_fold2.json") as f:
        saved = json.load(f)
    ref, _ = trajectory_reference(N, D, C, N, 100, 120)
    h1, h5 = hits(ref.logits, y2)
    assert saved == out and (saved["hits1"], saved["hits5"], saved["total"]) == (h1, h5, 120)
    assert saved["acc1"] == pytest.approx(100.0 * h1 / 120) and saved["steps"] == 100 and saved["bad_rows"] == 0
    assert saved["train_loss"] == pytest.approx(ref.loss_trace[-1], abs=1e-5)
    line = f"Linear probe steps=100 lr=0.125: Acc@1 = {saved['acc1']:.2f}% ({h1}/120), Acc@5 = {saved['acc5']:.2f}% ({h5}/120)"
    assert line in caplog.text
    out = linear_probe.main(["--features", str(tmp_path), "--fold", "2", "--steps", "10", "--batch", "64", "--lr", "0.05", "--wd", "0",
                             "--scale", "4", "--no-normalize"])
    assert (out["steps"], out["batch"], out["lr"], out["weight_decay"], out["scale"], out["normalize"]) == (10, 64, 0.05, 0.0, 4.0, False)
