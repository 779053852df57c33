"""GPU: rsp_linear_probe_fit / rsp_linear_probe_logits against the fp64 rule (linear_probe.probe_reference) -- one step across the
tile edges on both paths, the seeded trajectories, continuation, determinism and capture, guarded memory, non-finite values, the
workspace -- and the pretext driver's monitor."""
import ctypes
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from guarded import Guarded
from probe_util import GATE, TRAJECTORIES, case_inputs, check, hits, step_reference, step_state, trajectory_reference
from rspnet_amd import _lib, linear_probe, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, C, D): N in {1, 63, 64, 65, 129} around the 64-row tile, C in {1, 2, 5, 101, 128, 129, 256} (fused: below, at and across the
# 128- and 256-wide class tiles) and {257, 300} (general), D in {2, 30, 34, 200} (below, at and across a 32-wide k chunk and a
# 128-wide D tile); every value at least twice
STEP_CASES = [(1, 1, 2), (129, 1, 200), (63, 2, 30), (129, 2, 34), (64, 5, 34), (65, 5, 2), (1, 101, 34), (129, 101, 200),
              (65, 128, 200), (64, 128, 30), (64, 129, 2), (63, 129, 30), (63, 256, 200), (129, 256, 34), (65, 257, 30),
              (129, 257, 200), (129, 300, 34), (64, 300, 2)]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


class general_path:
    """The library's A/B switch: the four-launch path at any C."""

    def __enter__(self):
        os.environ["RSP_PROBE_GENERAL"] = "1"

    def __exit__(self, *exc):
        del os.environ["RSP_PROBE_GENERAL"]


def one_step(N, C, D):
    x, y, _, _ = case_inputs(N, D, C)
    w0, b0, m0 = step_state(N, D, C)
    w, b, mom = dev(w0), dev(b0), dev(m0)
    lr = torch.tensor([9.0, 0.125], device=DEV)
    trace, counts = ops.backend().linear_probe_fit(dev(x), dev(y), w, b, mom, lr, 1, N, first_step=1)
    return w.cpu().numpy(), b.cpu().numpy(), trace.cpu().numpy(), mom.cpu().numpy(), counts.cpu().tolist()


@pytest.mark.parametrize("case", STEP_CASES, ids=str)
def test_one_step_matches_fp64_reference(case):
    """One full-batch step from a random nonzero state with first_step = 1 (the momentum term is live): W, b, mom and the loss."""
    N, C, D = case
    w, b, trace, mom, counts = one_step(N, C, D)
    check(w, b, trace, step_reference(N, D, C), f"step {case}", mom=mom)
    assert counts == [N, 0]


@pytest.mark.parametrize("case", [(129, 101, 200), (1, 101, 34), (65, 5, 2)], ids=str)
def test_one_step_on_the_general_path_below_257_classes(case):
    N, C, D = case
    with general_path():
        w, b, trace, mom, counts = one_step(N, C, D)
    check(w, b, trace, step_reference(N, D, C), f"general step {case}", mom=mom)


def fit_from_zeros(x, y, C, batch, steps, first_step=0, state=None, lr=None, **kw):
    D = x.shape[1]
    w, b, mom = state if state is not None else (torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV),
                                                  torch.zeros(C * D + C, device=DEV))
    lr = dev(linear_probe.lr_schedule(0.125, 100 if steps < 100 else steps)) if lr is None else lr
    trace, counts = ops.backend().linear_probe_fit(x, y, w, b, mom, lr, steps, batch, first_step=first_step, **kw)
    return w, b, mom, trace, counts


@pytest.mark.parametrize("case", TRAJECTORIES, ids=str)
def test_trajectory_matches_fp64_reference(case):
    """The CPU suite's trajectory cases on the device at the same gates; the predictions on the training rows are the reference's on
    every row, and rsp_linear_probe_logits + rsp_xent_metrics count the reference's hits on a held-out set from the same means."""
    N, D, C, batch, steps = case
    x, y, x2, y2 = case_inputs(N, D, C, 200)
    ref, zref = trajectory_reference(N, D, C, batch, steps, 200)
    w, b, mom, trace, counts = fit_from_zeros(dev(x), dev(y), C, batch, steps)
    check(w.cpu().numpy(), b.cpu().numpy(), trace.cpu().numpy(), ref, f"device {case}")
    assert counts.tolist() == [N, 0]
    probe = linear_probe.Probe(w, b, trace, counts, True, 8.0)
    z = linear_probe.logits(probe, dev(x))
    assert np.array_equal(z.argmax(dim=1).cpu().numpy(), zref.argmax(axis=1))
    res = linear_probe.evaluate(probe, dev(x2), dev(y2))
    assert res["hits"] == hits(ref.logits, y2) and res["n"] == 200
    zz = np.take_along_axis(ref.logits, np.asarray(y2)[:, None], axis=1)[:, 0]
    want = float((np.log(np.exp(ref.logits - ref.logits.max(axis=1, keepdims=True)).sum(axis=1)) + ref.logits.max(axis=1) - zz).mean())
    assert res["loss"] == pytest.approx(want, abs=GATE)


def test_continuation_gives_the_bits_of_one_call():
    N, D, C, batch = 300, 34, 7, 64
    x, y, _, _ = case_inputs(N, D, C)
    xd, yd = dev(x), dev(y)
    whole = fit_from_zeros(xd, yd, C, batch, 100)
    first = fit_from_zeros(xd, yd, C, batch, 60)
    second = fit_from_zeros(xd, yd, C, batch, 40, first_step=60, state=first[:3])
    for a, b in zip(whole[:3], second[:3]):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(torch.cat([first[3], second[3]])), bits(whole[3]))


@pytest.mark.parametrize("case", [(300, 34, 7, 64), (300, 70, 300, 256)], ids=str)
def test_same_bits_over_runs_and_under_capture(case):
    """Three eager runs, one on a side stream, then the whole fit captured as one linear graph on one stream and replayed twice."""
    N, D, C, batch = case
    steps = 12
    x, y, _, _ = case_inputs(N, D, C)
    xd, yd, lr = dev(x), dev(y), dev(linear_probe.lr_schedule(0.125, steps))
    eager = fit_from_zeros(xd, yd, C, batch, steps, lr=lr)
    for _ in range(2):
        again = fit_from_zeros(xd, yd, C, batch, steps, lr=lr)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(eager, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = fit_from_zeros(xd, yd, C, batch, steps, lr=lr)
    side.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(eager, other))
    state = (torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C * D + C, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = fit_from_zeros(xd, yd, C, batch, steps, state=state, lr=lr)
    for _ in range(2):
        for t in cap[:3]:
            t.zero_()
        cap[3].fill_(-1.0)
        cap[4].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(eager, cap))


@pytest.mark.parametrize("case", [(129, 34, 7, 64), (300, 70, 300, 256)], ids=str)
def test_guarded_memory(case):
    """Every operand, output and the workspace inside 0xFF-filled allocations at the alignment the header promises: x (row pitch D + 2,
    the gap is NaN), y, w and the workspace on 8 bytes and not 16, b, mom and lr on 4 bytes and not 8.  No byte outside them
    changes, x, y and lr do not change, every element of w, b, mom, loss_trace and counts is written, and the gap's NaNs reach no
    output.  Then the same for the logits call."""
    N, D, C, batch = case
    steps = 3
    x, y, _, _ = case_inputs(N, D, C)
    ref = linear_probe.probe_reference(x, y, C, linear_probe.lr_schedule(0.125, steps), steps, batch)
    be = ops.backend()
    with Guarded(DEV, skew=8) as G:
        wide = G.alloc((N, D + 2), name="wide x")
        wide[:, :D] = dev(x)
        xd = wide[:, :D]
        before = wide.clone()
        yd = G.put(torch.from_numpy(np.array(y)))
        w = G.alloc((C, D), name="w")
        b = G.alloc((C + 1,), name="b")[1:]
        mom = G.alloc((C * D + C + 1,), name="mom")[1:]
        lr = G.put(torch.from_numpy(np.concatenate([[0.0], linear_probe.lr_schedule(0.125, steps)]).astype(np.float32)))[1:]
        assert xd.data_ptr() % 16 == 8 and w.data_ptr() % 16 == 8 and yd.data_ptr() % 16 == 8 and xd.stride(0) == D + 2
        assert b.data_ptr() % 8 == 4 and mom.data_ptr() % 8 == 4 and lr.data_ptr() % 8 == 4
        w.zero_()
        b.zero_()
        # mom stays 0xFF: step 0 must not read it (first_step + t == 0 writes d), and must write every element
        trace, counts = be.linear_probe_fit(xd, yd, w, b, mom, lr, steps, batch)
        G.check()
        kinds = sorted(blk.kind for blk in G.blocks)
        assert kinds == ["input", "input", "operand", "operand", "operand", "operand", "output", "output", "workspace"], kinds
        assert torch.equal(bits(wide), bits(before)) and bool((wide.view(torch.int32)[:, D:] == -1).all())
        assert counts.tolist() == [N, 0]
        got = (w.cpu().numpy(), b.cpu().numpy(), trace.cpu().numpy(), mom.cpu().numpy())
        probe = linear_probe.Probe(w, b, trace, counts, True, 8.0)
        z = be.linear_probe_logits(xd, w, b)
        G.check()
        assert torch.equal(bits(wide), bits(before))
        z = z.cpu().numpy()
    assert not any(np.isnan(a).any() for a in got) and not np.isnan(z).any()
    check(got[0], got[1], got[2], ref, f"guarded {case}", mom=got[3])
    zref = linear_probe.reference_logits(ref.w, ref.b, x)
    assert float(np.abs(z - zref).max()) <= GATE * float(np.abs(zref).max())


def test_invalid_rows_take_part_in_nothing():
    """A zero row, a row with a NaN, a row with an Inf and the labels -1 and C -- rows 255 and 256, the last lane of one 256-row trip of
    the compaction and the first lane of the next, among them --, with batch = N: W, b and loss_trace are, to the bit,
    those of the fit on the array without the rows -- on both paths; counts says how many there were; their logits are NaN."""
    N, D, C = 300, 34, 7
    x, y, _, _ = case_inputs(N, D, C)
    x, y = np.array(x), np.array(y)
    bad = [0, 63, 64, 200, 255, 256, N - 1]
    nb = len(bad)
    x[0] = 0
    x[63, D - 1] = np.nan
    x[64, 0] = np.inf
    y[200] = -1
    x[255, 1] = -np.inf
    y[256] = -1
    y[N - 1] = C
    ref = linear_probe.probe_reference(x, y, C, linear_probe.lr_schedule(0.125, 100), 100, N)
    for forced in (False, True):
        if forced:
            os.environ["RSP_PROBE_GENERAL"] = "1"
        try:
            got = fit_from_zeros(dev(x), dev(y), C, N, 100)
            want = fit_from_zeros(dev(np.delete(x, bad, axis=0)), dev(np.delete(y, bad)), C, N - nb, 100)
        finally:
            os.environ.pop("RSP_PROBE_GENERAL", None)
        assert got[4].tolist() == [N - nb, nb] and want[4].tolist() == [N - nb, 0]
        for a, b in zip(got[:4], want[:4]):
            assert torch.equal(bits(a), bits(b))
        check(got[0].cpu().numpy(), got[1].cpu().numpy(), got[3].cpu().numpy(), ref, f"seven invalid rows (general: {forced})")
    probe = linear_probe.Probe(got[0], got[1], got[3], got[4], True, 8.0)
    z = linear_probe.logits(probe, dev(x))
    assert torch.isnan(z).any(dim=1).nonzero().reshape(-1).tolist() == [0, 63, 64, 255] and bool(torch.isnan(z[[0, 63, 64, 255]]).all())
    res = linear_probe.evaluate(probe, dev(x), dev(y))
    assert res["hits"][0] == N - nb and res["rank"][bad].tolist() == [C] * nb
    # a chunk without a valid row: loss 0, only the weight decay moves the state
    w0, b0 = torch.full((C, D), 0.5, device=DEV), torch.full((C,), -0.25, device=DEV)
    out = fit_from_zeros(dev(x), torch.full((N,), C, dtype=torch.int64, device=DEV), C, N, 2, state=(w0, b0, torch.zeros(C * D + C, device=DEV)),
                         lr=torch.full((2,), 0.5, device=DEV))
    r0 = linear_probe.probe_reference(x, np.full(N, C), C, [0.5, 0.5], 2, N, w0=np.full((C, D), 0.5), b0=np.full(C, -0.25))
    assert out[3].tolist() == [0.0, 0.0] and out[4].tolist() == [0, N]
    assert np.allclose(out[0].cpu().numpy(), r0.w, rtol=1e-6) and np.allclose(out[1].cpu().numpy(), r0.b, rtol=1e-6)


def test_a_nan_learning_rate_propagates_from_its_step_on():
    N, D, C = 129, 30, 5
    x, y, _, _ = case_inputs(N, D, C)
    lr = linear_probe.lr_schedule(0.125, 10)
    clean = fit_from_zeros(dev(x), dev(y), C, 64, 10, lr=dev(lr))
    lr[5] = np.nan
    got = fit_from_zeros(dev(x), dev(y), C, 64, 10, lr=dev(lr))
    trace = got[3].cpu().numpy()
    # the loss of step t is formed before its update: steps 0 .. 5 are the clean run's, to the bit; from step 6 on W is NaN
    assert np.array_equal(trace[:6], clean[3].cpu().numpy()[:6]) and np.isnan(trace[6:]).all()
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[1]).all()) and got[4].tolist() == [N, 0]


def test_workspace_one_byte_short_launches_nothing():
    N, D, C = 129, 34, 7
    x, y, _, _ = case_inputs(N, D, C)
    xd, yd = dev(x), dev(y)
    w, b, mom = (torch.full(s, 3.0, device=DEV) for s in ((C, D), (C,), (C * D + C,)))
    out, counts, lr = torch.full((2,), 3.0, device=DEV), torch.full((2,), 3, dtype=torch.int32, device=DEV), torch.full((2,), 0.1, device=DEV)
    lib = _lib.load()
    need = lib.rsp_linear_probe_workspace(N, D, C, 64)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.rsp_linear_probe_fit(p(xd), D, N, D, p(yd), C, 64, 0, 2, p(lr), 0.9, 1e-4, 1, 8.0, p(w), p(b), p(mom), p(out), p(counts),
                                  p(ws), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -2 and lib.rsp_last_error() == b"rsp_linear_probe_fit: workspace too small"
    assert all(bool((t == 3).all()) for t in (w, b, mom, out, counts)) and not bool(ws.any())


# ---- the monitor ---------------------------------------------------------------------------------------------------------
def test_monitor_run_leaves_the_model_and_the_generators_alone():
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory
    torch.manual_seed(3)
    model = ModelFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=DEV)
    net = model.module
    net.train()
    net.encoder_k.eval()                                   # a mixed set of flags: every module gets its own back
    mon = linear_probe.LinearProbeMonitor(every=1, num_epochs=1, num_classes=3, bank_samples=24, query_samples=12, batch_size=4, steps=20)
    bank, query = mon.build_loaders(16, 32, DEV, seed=0)
    before = {n: t.clone() for n, t in net.state_dict().items()}
    flags = [m.training for m in net.modules()]
    states = (random.getstate(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(DEV).clone())
    out = mon.run(model, bank, query)
    assert set(out) == {"acc1", "acc5", "loss", "train_loss", "n_bank", "n_query", "bad_rows", "seconds"}
    assert out["n_bank"] == 24 and out["n_query"] == 12 and 0 <= out["acc1"] <= out["acc5"] <= 100 and np.isfinite(out["loss"])
    assert out["bad_rows"] == 0 and out["train_loss"] < np.log(3)
    after = net.state_dict()
    assert list(after) == list(before)
    for n, t in after.items():
        assert torch.equal(t, before[n]), n
    assert [m.training for m in net.modules()] == flags
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    assert torch.equal(torch.cuda.get_rng_state(DEV), states[2])
    again = mon.run(model, bank, query)
    assert all(again[k] == out[k] for k in out if k != "seconds")
    mon_k = linear_probe.LinearProbeMonitor(every=1, num_epochs=1, num_classes=3, encoder="k", bank_samples=24, query_samples=12,
                                            batch_size=4, steps=5, batch=16)
    assert 0 <= mon_k.run(model, bank, query)["acc1"] <= 100


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
    scalar and the backend's linear_probe_fit is never called; both runs train the same model, checkpoint for checkpoint."""
    from rspnet_amd.pretrain import main_worker
    be = ops.backend()
    calls = []
    inner = be.linear_probe_fit

    def counted(x, *a, **kw):
        calls.append(tuple(x.shape))
        return inner(x, *a, **kw)
    be.linear_probe_fit = counted
    try:
        keys = {"probe_monitor": {"every": 2, "num_classes": 3, "bank_samples": 24, "query_samples": 12, "batch_size": 4, "steps": 20}}
        main_worker(0, _args(tmp_path, keys, "with"), "")
        with_calls = list(calls)
        del calls[:]
        main_worker(0, _args(tmp_path, {}, "without"), "")
        without_calls = list(calls)
    finally:
        del be.linear_probe_fit
    lines = {name: [json.loads(l) for l in open(tmp_path / name / "exp" / "run_0_t" / "scalars.jsonl")] for name in ("with", "without")}
    assert len(lines["with"]) == 2 and len(lines["without"]) == 2
    first, second = lines["with"]
    assert not any(k.startswith("probe_") for k in first)
    assert sorted(k for k in second if k.startswith("probe_")) == ["probe_acc1", "probe_acc5", "probe_loss"]
    assert 0 <= second["probe_acc1"] <= second["probe_acc5"] <= 100 and np.isfinite(second["probe_loss"])
    assert len(with_calls) == 1 and with_calls[0][0] == 24 and without_calls == []
    assert not any(k.startswith("probe_") for rec in lines["without"] for k in rec)
    for a, b in zip(lines["with"], lines["without"]):
        assert {k: v for k, v in a.items() if not k.startswith("probe_")} == b      # the step's numbers are unchanged
    a = torch.load(tmp_path / "with" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    b = torch.load(tmp_path / "without" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n
