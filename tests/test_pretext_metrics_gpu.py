"""GPU: rsp_pretext_metrics (pretext_metrics.hip) and the pretext driver's meters.  The rank of the positive is a count and every
accuracy is two fp32 operations, so every comparison is exact equality against the torch restatement evaluated on the CPU
(rspnet_amd.pretrain.pretext_accuracy; tests/test_pretext_metrics_cpu.py holds that one against the reference's own functions)."""
import json
import logging
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BS = (1, 3, 32)
K1S = (5, 63, 64, 65, 257, 16385)      # odd K1: rows that start off a 16-byte boundary (scalar head and tail); 16385: the shipped size
MISS = 0x7fffffff


def dev():
    return torch.device("cuda", 0)


def backend():
    from rspnet_amd import ops
    be = ops.backend()
    assert be.name == "hip"
    return be


# Where call() places its operands on the device.  tests/test_guarded_downstream_gpu.py runs the bodies with these two pointed at
# guarded allocations (tests/guarded.py): place() for inputs, place_empty() for what the kernel writes.
def place(t):
    return t.to(dev())


def place_empty(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=dev())


def restate(l1, l2, lp, ln):
    from rspnet_amd.pretrain import pretext_accuracy
    return pretext_accuracy((l1, l2), (lp.view(-1, 1), ln.view(-1, 1)))


def ranks_of(x):
    """rank = #{c : v[c] > v[0]}; MISS for a NaN positive (int32, as the kernel leaves it in its workspace)."""
    r = (x > x[:, :1]).sum(dim=1)
    return torch.where(x[:, 0] != x[:, 0], torch.full_like(r, MISS), r).to(torch.int32)


def call(be, l1, l2, lp, ln, losses=None, meters=None):
    """The entry point itself, with a workspace of the test's own: returns (acc, ranks of the 2 * B rows) on the host."""
    B, K1 = l1.shape
    d = [place(t.contiguous()) for t in (l1, l2, lp.reshape(-1), ln.reshape(-1))]
    ls = None if losses is None else place(losses)
    acc = place_empty(5).fill_(-1.0)
    wsb = be.lib.rsp_pretext_metrics_workspace(B)
    assert wsb == 8 * B
    ws = place_empty(2 * B, dtype=torch.int32).fill_(-7)
    rc = be.lib.rsp_pretext_metrics(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, K1,
                                    None if ls is None else ls.data_ptr(), acc.data_ptr(),
                                    None if meters is None else meters.data_ptr(), ws.data_ptr(), wsb,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, be.lib.rsp_last_error()
    torch.cuda.synchronize()
    return acc.cpu(), ws.cpu()


def check(be, l1, l2, lp, ln):
    acc, ranks = call(be, l1, l2, lp, ln)
    want = restate(l1, l2, lp, ln)
    print(f"B={l1.shape[0]} K1={l1.shape[1]} acc {acc.tolist()} want {want.tolist()}")
    assert torch.equal(ranks, torch.cat([ranks_of(l1), ranks_of(l2)]))
    assert torch.equal(acc, want)
    return acc, ranks


def draw(B, K1, seed):
    g = torch.Generator().manual_seed(seed)
    l1, l2 = torch.randn(B, K1, generator=g), torch.randn(B, K1, generator=g)
    lp, ln = torch.randn(B, generator=g), torch.randn(B, generator=g)
    losses = torch.rand(3, generator=g) * 10
    return l1, l2, lp, ln, losses


@pytest.mark.parametrize("K1", K1S)
@pytest.mark.parametrize("B", BS)
def test_shapes(B, K1):
    l1, l2, lp, ln, _ = draw(B, K1, 1000 * B + K1)
    for m in (l1, l2):
        assert not bool((m[:, 1:] == m[:, :1]).any())      # no column equals its row's positive
    assert not bool((lp == ln).any())
    check(backend(), l1, l2, lp, ln)


def positions(K1):
    """Columns that sit at the ends of a row and on both sides of a wavefront's (64 lanes x 4 floats) and a workgroup's (256 x 4)
    stride, for every head length 0..3 a misaligned row can have."""
    cand = [1, K1 - 1, 2, K1 - 2, 3, 4, 63, 64, 65] + list(range(253, 261)) + list(range(1021, 1029)) + [K1 - 3, K1 - 4, 2048, 4099]
    out = []
    for c in cand:
        if 1 <= c < K1 and c not in out:
            out.append(c)
    return out


def planted_rows(K1, counts, value, fill=-1.0):
    """One row per (count, rotation): positive 0, `fill` elsewhere, `value` in `count` columns taken from positions(K1)."""
    pos = positions(K1)
    rows, want = [], []
    for n in counts:
        for rot in range(0, len(pos), 3):
            row = torch.full((K1,), fill)
            row[0] = 0.0
            if n >= K1 - 1:
                row[1:] = value
            else:
                order = pos[rot:] + pos[:rot]
                row[torch.tensor(order[:n], dtype=torch.long)] = value
            rows.append(row)
            want.append(K1 - 1 if n >= K1 - 1 else min(n, len(pos)))
    return torch.stack(rows), want


@pytest.mark.parametrize("K1", K1S)
def test_boundaries(K1):
    """Exactly 0, 1, 4, 5 and K1 - 1 columns above the positive."""
    x, want = planted_rows(K1, (0, 1, 4, 5, K1 - 1), 1.0)
    assert K1 == 5 or len(positions(K1)) >= 5
    B = x.shape[0]
    lp = torch.arange(B, dtype=torch.float32)
    ln = lp.flip(0)
    acc, ranks = check(backend(), x, x.flip(0), lp, ln)
    assert ranks[:B].tolist() == want and ranks[B:].tolist() == want[::-1]
    h1, h5 = sum(w == 0 for w in want), sum(w < 5 for w in want)
    per = np.float32(100.0 / B)
    assert acc.tolist() == [float(np.float32(h) * per) for h in (h1, h5, h1, h5, (B + 1) // 2)]


@pytest.mark.parametrize("K1", (5, 65, 16385))
def test_ties(K1):
    """Duplicates of the positive's value do not count, alone or next to larger columns; lposM == lnegM is a hit."""
    dup, _ = planted_rows(K1, (1, 3, 5, K1 - 1), 0.0)                # duplicates only: rank 0
    both, want = planted_rows(K1, (1, 4, 5), 1.0, fill=0.0)          # every other column a duplicate, n larger
    B = dup.shape[0]
    both = both[:B] if both.shape[0] >= B else torch.cat([both, dup[:B - both.shape[0]]])
    want = (want + [0] * B)[:B]
    lp = torch.tensor([0.5, -1.0, 2.0] * B)[:B]
    acc, ranks = check(backend(), dup, both, lp, lp.clone())
    assert ranks[:B].tolist() == [0] * B and ranks[B:].tolist() == want
    full = float(np.float32(B) * np.float32(100.0 / B))
    assert acc[0] == full and acc[1] == full and acc[4] == full


def test_non_finite():
    K1 = 65
    nan, inf = float("nan"), float("inf")
    x = torch.full((4, K1), -1.0)
    x[:, 0] = 0.0
    x[0, 0] = nan                      # NaN positive: a miss
    x[1, [1, 7, 64]] = nan             # NaN elsewhere does not count: rank 0
    x[2, 3] = inf                      # +inf elsewhere counts: rank 1
    x[3, 0] = -inf                     # -inf positive, finite others: rank K1 - 1
    lp = torch.tensor([nan, 1.0, 1.0, 0.0])
    ln = torch.tensor([0.0, nan, 1.0, 1.0])
    acc, ranks = check(backend(), x, x.flip(0), lp, ln)
    assert ranks.tolist() == [MISS, 0, 1, K1 - 1, K1 - 1, 1, 0, MISS]
    assert acc.tolist() == [25.0, 50.0, 25.0, 50.0, 25.0]


def read_meters(buf):
    h = buf.cpu().numpy()
    return h[0:32].view(np.float32).copy(), h[32:64].view(np.float32).copy(), h[64:96].view(np.int32).copy()


def test_meters():
    """Three calls on one struct against a numpy fp32 restatement of AverageMeter.update; the torch path gives the same buffer."""
    from rspnet_amd.pretrain import PretextMeters
    be = backend()
    hip, tor = PretextMeters(dev()), PretextMeters(dev())
    assert hip.buf.numel() == 96
    total, count = np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.int32)
    for i, (B, K1) in enumerate(((3, 65), (32, 257), (1, 63))):
        l1, l2, lp, ln, losses = draw(B, K1, 50 + i)
        l1[:, 0] += 2.5      # hit rates away from zero
        l2[:, 0] += 1.5
        want = restate(l1, l2, lp, ln)
        acc, _ = call(be, l1, l2, lp, ln, losses, hip.buf)
        bare, _ = call(be, l1, l2, lp, ln)                           # meters = NULL: acc is still written
        assert torch.equal(acc, want) and torch.equal(bare, want)
        v = np.array([float(t) for t in (losses[0], losses[1], want[0], want[1], want[2], want[3], losses[2], want[4])],
                     dtype=np.float32)
        total = (total + (v * np.float32(B)).astype(np.float32)).astype(np.float32)
        count += B
        val, msum, mcount = read_meters(hip.buf)
        print(f"call {i}: val {val.tolist()} sum {msum.tolist()} count {mcount.tolist()}")
        assert np.array_equal(val, v) and np.array_equal(msum, total) and np.array_equal(mcount, count)
        d = [t.to(dev()) for t in (losses[0], losses[1], want[0], want[1], want[2], want[3], losses[2], want[4])]
        tor.update(d, B)
        assert torch.equal(tor.buf, hip.buf)
        # the ops wrapper: same call, acc returned as a device tensor
        again = be.pretext_metrics(l1.to(dev()), l2.to(dev()), lp.to(dev()), ln.to(dev()), losses.to(dev()))
        assert torch.equal(again.cpu(), want)
    stats = hip.read()
    assert stats["loss"]["count"] == 36 and stats["acc1_M"]["avg"] == float(total[7] / np.float32(36))


def test_errors():
    """Argument checks: RSP_EINVAL with text, nothing launched."""
    from rspnet_amd import _lib
    be = backend()
    lib = be.lib
    z = torch.zeros((2, 8), device=dev())
    v = torch.zeros(2, device=dev())
    acc = torch.full((5,), -1.0, device=dev())
    ws = torch.zeros(64, dtype=torch.int32, device=dev())
    args = lambda B, K1, wsb: (z.data_ptr(), z.data_ptr(), v.data_ptr(), v.data_ptr(), B, K1, None, acc.data_ptr(), None, ws.data_ptr(),
                               wsb, None)
    assert lib.rsp_pretext_metrics(*args(2, 4, 256)) == -1 and b"K1" in lib.rsp_last_error()
    assert lib.rsp_pretext_metrics(*args(0, 8, 256)) == -1 and b"B >= 1" in lib.rsp_last_error()
    assert lib.rsp_pretext_metrics_workspace(2) == 16 and lib.rsp_pretext_metrics_workspace(0) == 0
    assert lib.rsp_pretext_metrics(*args(2, 8, 15)) == -1 and b"workspace" in lib.rsp_last_error()
    torch.cuda.synchronize()
    assert acc.tolist() == [-1.0] * 5
    with pytest.raises(_lib.RspError):
        be.pretext_metrics(torch.zeros((2, 4), device=dev()), torch.zeros((2, 4), device=dev()), v, v, torch.zeros(3, device=dev()))
    with pytest.raises(_lib.RspError):
        be.pretext_metrics(z, z, v, v, torch.zeros(3, device=dev()), torch.zeros(36, dtype=torch.uint8, device=dev()))


def test_captured_once_and_replayed():
    from rspnet_amd.pretrain import PretextMeters
    be = backend()
    B, K1 = 3, 257
    inputs = [draw(B, K1, 70 + i) for i in range(3)]
    for l1, l2, *_ in inputs:
        l1[:, 0] += 2.5
        l2[:, 0] += 2.0
    static = [t.to(dev()).clone() for t in inputs[0]]
    meters = PretextMeters(dev())
    eager = []
    for case in inputs:
        eager.append(be.pretext_metrics(*[t.to(dev()) for t in case], meters.buf).cpu())
    torch.cuda.synchronize()
    eager_buf = meters.buf.cpu()
    meters.reset()
    be.pretext_metrics(*static, meters.buf)                          # first call's buffers, eagerly
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = be.pretext_metrics(*static, meters.buf)
    for case, want in zip(inputs[1:], eager[1:]):
        for s, t in zip(static, case):
            s.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.cpu(), want)
    assert meters.count.tolist() == [3 * B] * 8                     # one eager call, two replays
    assert torch.equal(meters.buf.cpu(), eager_buf)
    assert [e.tolist() for e in eager] == [restate(*c[:4]).tolist() for c in inputs]


# ---- driver ---------------------------------------------------------------------------------------------------------------
def _args(tmp_path, **kw):
    cfg = json.load(open("rspnet_amd/config/pretrain/c3d.json"))
    cfg.update(batch_size=4, num_epochs="2", log_interval=2)
    cfg["moco"]["k"] = 64
    cfg["spatial_transforms"]["size"] = 32
    p = tmp_path / "cfg.json"
    json.dump(cfg, open(p, "w"))
    a = dict(config=str(p), ext_config=None, experiment_dir=str(tmp_path / "exp"), load_checkpoint=None, load_model=None,
             debug=False, world_size=1, seed=0, no_scale_lr=False, steps_per_epoch=3, run_dir=str(tmp_path / "exp" / "run_0_t"),
             cont=False)
    a.update(kw)
    return types.SimpleNamespace(**a), cfg


OLD_KEYS = ("loss", "loss_A", "loss_M", "acc1_A")
NEW_KEYS = ("acc5_A", "acc1_A_n", "acc5_A_n", "acc1_M")
TAGS = ("train/lr", "train/loss", "train/loss_A", "train/acc1_A", "train/acc5_A", "train/loss_M", "train/acc1_M")


def test_driver_two_epochs(tmp_path, monkeypatch, caplog):
    from rspnet_amd import ops, pretrain
    steps, reads = [], []
    orig = ops.HipOps.pretext_metrics

    def recording(self, l1, l2, lp, ln, losses, meters_buf=None):
        steps.append([t.detach().clone() for t in (l1, l2, lp, ln, losses)])
        return orig(self, l1, l2, lp, ln, losses, meters_buf)

    orig_read = pretrain.PretextMeters.read
    monkeypatch.setattr(ops.HipOps, "pretext_metrics", recording)
    monkeypatch.setattr(pretrain.PretextMeters, "read", lambda self: (reads.append(1), orig_read(self))[1])
    caplog.set_level(logging.INFO, logger="rspnet_amd.pretrain")
    args, _ = _args(tmp_path)
    stats = pretrain.main_worker(0, args, "")
    assert len(steps) == 6 and len(reads) == 4      # per epoch: one call per step; one read at the log line, one at the end
    B = 4
    meters = pretrain.PretextMeters("cpu")
    per_step = []
    for l1, l2, lp, ln, losses in (s for s in steps[3:]):
        l1, l2, lp, ln, losses = (t.cpu() for t in (l1, l2, lp, ln, losses))
        assert l1.shape == (B, 65)
        acc = restate(l1, l2, lp, ln)
        v = [losses[0], losses[1], acc[0], acc[1], acc[2], acc[3], losses[2], acc[4]]
        per_step.append([float(x) for x in v])
        meters.update(v, B)
    want = meters.read()
    print("stats", stats, "per step", per_step)
    for k in OLD_KEYS + NEW_KEYS:
        assert stats[k] == want[k]["avg"], k
    mean = np.mean(np.array(per_step, dtype=np.float64), axis=0)
    for k in OLD_KEYS:      # the meaning the keys had: the mean over the epoch's steps (fp32 sums of 3 terms: a few ulp)
        assert abs(stats[k] - mean[pretrain.PretextMeters.KEYS.index(k)]) <= 1e-6 * max(1.0, abs(stats[k])), k
    assert stats["clips_per_s"] > 0
    scalars = [json.loads(line) for line in open(tmp_path / "exp" / "run_0_t" / "scalars.jsonl")]
    assert len(scalars) == 2 and [s["epoch"] for s in scalars] == [0, 1]
    for s in scalars:
        assert set(s) == set(TAGS) | {"epoch"}
    assert scalars[1]["train/loss"] == stats["loss"] and scalars[1]["train/acc5_A"] == stats["acc5_A"]
    assert scalars[0]["train/lr"] > scalars[1]["train/lr"] > 0
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Train [")]
    assert len(lines) == 2 and lines[0].startswith("Train [0/2][1/3]\tLoss_A ") and lines[1].startswith("Train [1/2][1/3]\tLoss_A ")
    first, second, third = lines[1].split("\n")
    assert [p.split(" ")[0] for p in first.split("\t")[1:]] == ["Loss_A", "Acc@1_A", "Acc@5_A"]
    assert [p.split(" ")[0] for p in second.split("\t")] == ["Loss_M", "Acc@1_M"]
    assert [p.split(" ")[0] for p in third.split("\t")] == ["Acc@1_A_n", "Acc@5_A_n"]


def test_driver_validate_epoch(tmp_path):
    from rspnet_amd import pretrain
    from rspnet_amd.utils.moco import replace_moco_k_in_config
    args, cfg = _args(tmp_path, validate=True)
    replace_moco_k_in_config(cfg)
    torch.manual_seed(0)
    eng = pretrain.Engine(args, cfg, 0)
    before = {n: p.detach().clone() for n, p in eng.model.module.encoder_q.named_parameters()}
    ptr0 = int(eng.model.module.state_dict()["queue_ptr"].item())
    stats = eng.run()
    eng.model.sync_buffers()
    assert eng._stepper is None and eng.current_epoch == 0
    after = dict(eng.model.module.encoder_q.named_parameters())
    assert before and all(torch.equal(before[n], after[n]) for n in before)
    read = eng.meters.read()
    assert all(read[k]["count"] == 3 * 4 for k in pretrain.PretextMeters.KEYS)
    assert stats["loss"] == read["loss"]["avg"] and stats["loss"] == stats["loss"] and 0 <= stats["acc5_A"] <= 100
    state = eng.model.module.state_dict()
    assert (int(state["queue_ptr"].item()) - ptr0) % 64 == 12                       # the queue moved: three batches of four
    assert state["encoder_q.encoder.bn1.num_batches_tracked"].item() == 3           # so did the BatchNorm statistics
    assert not (tmp_path / "exp" / "checkpoint.pth.tar").exists()
