"""GPU: rsp_repr_stats (HipOps.repr_stats) against the fp64 restatement at the tile edges of its 64 x 128 x 32 walk, on a planted case
with exact answers, inside guarded memory, with invalid rows, over runs and under capture, once at the queue's size; the monitor
alone and inside the pretext driver."""
import json
import random
import types

import numpy as np
import pytest
import torch

from guarded import Guarded
from repr_util import GATE, case_input, case_reference, check
from rspnet_amd import _lib, ops, repr_stats

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# every N of 2, 63, 64, 65, 127, 128, 129, 193, 300 and every D of 2, 30, 32, 34, 70, 128: one row tile / two / a second column tile /
# a third, D below, at and above the 32-wide chunk and the 64- and 128-wide Gram tiles
CASES = [(2, 2), (63, 32), (64, 30), (65, 30), (127, 34), (128, 128), (129, 34), (129, 2), (193, 70), (300, 70), (300, 128)]
KINDS = {(65, 30): "offset", (300, 70): "offset"}      # (a common direction: sums that do not cancel)


def raw(res):
    """The three device outputs of one call, read once."""
    s = _lib.ReprSums.from_buffer_copy(res.sums.cpu().numpy().tobytes())
    return {"pair_exp": s.pair_exp, "pair_cos": s.pair_cos, "pair_cos2": s.pair_cos2, "rows_valid": s.rows_valid, "rows_bad": s.rows_bad,
            "gram": res.gram.cpu().numpy(), "colsum": res.colsum.cpu().numpy()}


def same_bits(a, b):
    return all(torch.equal(u.view(torch.uint8).reshape(-1), v.view(torch.uint8).reshape(-1)) for u, v in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_matches_fp64_reference(case):
    kind = KINDS.get(case, "normal")
    x = torch.from_numpy(case_input(*case, kind).copy()).to(DEV)
    got = raw(ops.backend().repr_stats(x, 2.0))
    check(got, case_reference(*case, kind), f"rsp_repr_stats {case} {kind}")
    assert np.array_equal(got["gram"], got["gram"].T)      # both triangles, from the same products in the same order


@pytest.mark.parametrize("case", [(65, 200), (40, 322)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_gram_wider_than_two_tiles(case):
    """D above 128: the 64 x 128 Gram tiles wholly below the diagonal are not computed; their elements are read from the mirror
    image (three and five a-tiles against two and three b-tiles, the last ones partial)."""
    x = torch.from_numpy(case_input(*case).copy()).to(DEV)
    got = raw(ops.backend().repr_stats(x, 2.0))
    check(got, case_reference(*case), f"rsp_repr_stats {case}")
    assert np.array_equal(got["gram"], got["gram"].T)


@pytest.mark.parametrize("N, D", [(2, 2), (63, 30), (64, 30), (65, 30), (127, 34), (128, 34), (129, 34), (193, 30), (300, 34), (300, 2)])
def test_planted_unit_rows_are_exact(N, D):
    """Rows e_(i mod D): every s is exactly 0 or 1, so pair_cos and pair_cos2 are the integer count of same-residue pairs -- a pair
    counted twice or not at all shows as a whole number -- and pair_exp is that count plus the other pairs times expf(-c)."""
    x = torch.zeros(N, D)
    x[torch.arange(N), torch.arange(N) % D] = 1.0
    t = 1.5
    got = raw(ops.backend().repr_stats(x.to(DEV), t))
    n_r = np.bincount(np.arange(N) % D, minlength=D)
    same = int((n_r * (n_r - 1) // 2).sum())
    rest = N * (N - 1) // 2 - same
    assert got["pair_cos"] == same and got["pair_cos2"] == same and (got["rows_valid"], got["rows_bad"]) == (N, 0)
    want = same + rest * float(np.exp(np.float32(-2.0 * t)))
    assert abs(got["pair_exp"] - want) <= 1e-6 * want
    assert np.array_equal(got["gram"], np.diag(n_r.astype(np.float64))) and np.array_equal(got["colsum"], n_r.astype(np.float64))


@pytest.mark.parametrize("N, D", [(129, 34), (300, 70)])
def test_guarded_memory(N, D):
    """x inside a 0xFF-filled allocation with row pitch D + 2 (the gap is NaN) and an 8-byte, not 16-byte, aligned base; sums, gram,
    colsum and the workspace in allocations of the same kind: no byte outside them changes, x does not change, gram and colsum --
    NaN before the call -- hold no NaN afterwards, and the gap's NaNs reach no output."""
    be = ops.backend()
    with Guarded(DEV, skew=8) as G:
        wide = G.alloc((N, D + 2), name="wide x")
        wide[:, :D] = torch.from_numpy(case_input(N, D).copy()).to(DEV)
        x = wide[:, :D]
        assert x.data_ptr() % 16 == 8 and x.stride(0) == D + 2
        before = wide.clone()
        res = be.repr_stats(x, 2.0)
        G.check()
        kinds = sorted(b.kind for b in G.blocks)
        assert kinds == ["operand", "output", "output", "output", "workspace"], kinds
        assert all(any(b.payload.data_ptr() == t.data_ptr() for b in G.blocks) for t in res)
        assert torch.equal(wide.view(torch.int32), before.view(torch.int32)) and bool((wide.view(torch.int32)[:, D:] == -1).all())
        got = raw(res)
    assert not np.isnan(got["gram"]).any() and not np.isnan(got["colsum"]).any()
    check(got, case_reference(N, D), f"guarded {N}x{D}")


def test_invalid_rows_take_part_in_nothing():
    N, D = 300, 70
    x = np.array(case_input(N, D))
    bad = [0, 63, 64, 200, 255, 256, 299]      # (255, 256: the last row of one 256-row stretch and the first of the next)
    x[0] = 0
    x[63, 69] = np.nan
    x[64, 0] = np.inf
    x[200] = np.nan
    x[255, 5] = np.inf
    x[256] = 0
    x[299, 31] = -np.inf
    ref = repr_stats.repr_reference(np.delete(x, bad, axis=0))
    got = raw(ops.backend().repr_stats(torch.from_numpy(x).to(DEV), 2.0))
    assert (got["rows_valid"], got["rows_bad"]) == (N - 7, 7)
    check(dict(got, rows_bad=0), ref, "seven invalid rows")
    out = repr_stats.repr_stats(torch.from_numpy(x).to(DEV))
    assert (out["rows"], out["bad_rows"]) == (N - 7, 7) and all(np.isfinite(v) for v in out.values())
    # fewer than two valid rows: the sums are zero, the uniformity is NaN
    one = repr_stats.repr_stats(torch.from_numpy(x[[0, 1, 200]]).to(DEV))
    assert np.isnan(one["uniformity"]) and np.isnan(one["mean_cos"]) and (one["rows"], one["bad_rows"]) == (1, 2)


def test_same_bits_over_runs_and_under_capture():
    be = ops.backend()
    x = torch.from_numpy(case_input(300, 70, "offset").copy()).to(DEV)
    eager = be.repr_stats(x, 2.0)
    again = be.repr_stats(x, 2.0)
    assert same_bits(eager, again)
    nogram = be.repr_stats(x, 2.0, want_gram=False)
    assert nogram.gram is None and nogram.colsum is None and same_bits(nogram[:1], eager[:1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = be.repr_stats(x, 2.0)
    for _ in range(2):
        for t in cap:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(cap, eager)


def test_queue_size_against_chunked_fp64():
    """N = 16384, D = 128: the pretext queue.  The reference is the rule composed from torch fp64 ops on the device, 1024 rows at a time."""
    N, D, t = 16384, 128, 2.0
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(N, D, device=DEV, generator=gen) + 0.3 * torch.randn(1, D, device=DEV, generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    got = raw(ops.backend().repr_stats(x, t))
    grown = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak growth {grown / 2**20:.1f} MiB vs {N * N * 4 / 2**20:.0f} MiB for the matrix")
    assert grown < N * N * 4 // 8
    ss = (x * x).sum(dim=1)
    inv = (1.0 / ss.sqrt()).double()
    xd = x.double()
    col = torch.arange(N, device=DEV)
    pe, pc, pc2 = (torch.zeros((), dtype=torch.float64, device=DEV) for _ in range(3))
    for r0 in range(0, N, 1024):
        s = (xd[r0:r0 + 1024] @ xd.t()) * inv[r0:r0 + 1024, None] * inv[None, :]
        keep = col[None, :] > col[r0:r0 + 1024, None]
        pe += torch.where(keep, torch.exp(2.0 * t * (s - 1.0)), torch.zeros_like(s)).sum()
        pc += torch.where(keep, s, torch.zeros_like(s)).sum()
        pc2 += torch.where(keep, s * s, torch.zeros_like(s)).sum()
    xh = (x * (1.0 / ss.sqrt())[:, None]).double()
    ref = {"pair_exp": float(pe), "pair_cos": float(pc), "pair_cos2": float(pc2), "rows_valid": N, "rows_bad": 0,
           "gram": (xh.t() @ xh).cpu().numpy(), "colsum": xh.sum(dim=0).cpu().numpy()}
    check(got, ref, "queue size 16384 x 128")


# ---- the monitor ---------------------------------------------------------------------------------------------------------
def test_monitor_run_leaves_the_model_and_the_generators_alone():
    from model_util import make_cfg
    from rspnet_amd.moco import ModelFactory
    torch.manual_seed(3)
    model = ModelFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=DEV)
    net = model.module
    before = {n: t.clone() for n, t in net.state_dict().items()}
    flags = [m.training for m in net.modules()]
    states = (random.getstate(), torch.get_rng_state().clone(), torch.cuda.get_rng_state(DEV).clone())
    mon = repr_stats.ReprMonitor(every=1, num_epochs=1)
    out = mon.run(model)
    assert set(out) == {"uniformity", "mean_cos", "mean_cos2", "effective_rank", "dim_std_min", "dim_std_mean", "rows", "bad_rows", "seconds"}
    K, dim = net.queue.shape[1], net.queue.shape[0]
    assert (out["rows"], out["bad_rows"]) == (K, 0) and 1 <= out["effective_rank"] <= min(K, dim) and out["uniformity"] < 0
    want = repr_stats.summarize(repr_stats.repr_reference(net.queue.t().cpu().numpy()))
    assert out["uniformity"] == pytest.approx(want["uniformity"], abs=1e-4)
    # K = 64 rows in 128 dimensions: 64 singular values are zero, and a Gram error of eps * max|gram| moves each by up to sqrt(eps) --
    # at the fp32 products' 2e-7 that is 64 * 4e-4 of a total mass of about 64, a shift of the rank of some 1e-3 relative
    assert out["effective_rank"] == pytest.approx(want["effective_rank"], rel=2e-2)
    after = net.state_dict()
    assert list(after) == list(before)
    for n, t in after.items():
        assert torch.equal(t, before[n]), n
    assert [m.training for m in net.modules()] == flags
    assert random.getstate() == states[0] and torch.equal(torch.get_rng_state(), states[1])
    assert torch.equal(torch.cuda.get_rng_state(DEV), states[2])
    again = mon.run(model)
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
    """Two epochs, the monitor every second one: its scalars are in the second line only; with the kNN monitor due in the same epoch
    the bank features go through the same call.  Without the key no line carries such a scalar and the backend's repr_stats is never
    called; both runs train the same model, checkpoint for checkpoint."""
    from rspnet_amd.pretrain import main_worker
    be = ops.backend()
    calls = []
    inner = be.repr_stats

    def counted(x, *a, **kw):
        calls.append(tuple(x.shape))
        return inner(x, *a, **kw)
    be.repr_stats = counted
    try:
        keys = {"repr_monitor": {"every": 2, "t": 2.0},
                "knn_monitor": {"every": 1, "k": 8, "num_classes": 3, "bank_samples": 24, "query_samples": 12, "batch_size": 4}}
        main_worker(0, _args(tmp_path, keys, "with"), "")
        with_calls = list(calls)
        del calls[:]
        main_worker(0, _args(tmp_path, {}, "without"), "")
        without_calls = list(calls)
    finally:
        del be.repr_stats
    lines = {name: [json.loads(l) for l in open(tmp_path / name / "exp" / "run_0_t" / "scalars.jsonl")] for name in ("with", "without")}
    assert len(lines["with"]) == 2 and len(lines["without"]) == 2
    own = ["repr/uniformity", "repr/mean_cos", "repr/effective_rank", "repr/dim_std_min", "repr/bad_rows"]
    bank = ["repr/bank_uniformity", "repr/bank_effective_rank", "repr/bank_dim_std_min"]
    first, second = lines["with"]
    assert not any(k.startswith("repr/") for k in first) and "knn/acc1" in first
    assert sorted(k for k in second if k.startswith("repr/")) == sorted(own + bank)
    assert all(np.isfinite(second[k]) for k in own + bank) and second["repr/bad_rows"] == 0 and second["repr/uniformity"] < 0
    assert len(with_calls) == 2 and with_calls[0][0] == 64 and with_calls[1][0] == 24      # the queue (K rows), then the bank
    assert not any(k.startswith("repr/") for rec in lines["without"] for k in rec) and without_calls == []
    a = torch.load(tmp_path / "with" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    b = torch.load(tmp_path / "without" / "exp" / "checkpoint.pth.tar", weights_only=False)["model"]
    assert list(a) == list(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n
