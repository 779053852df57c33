"""GPU: rsp_xent_metrics (classify.hip) against an fp64 numpy restatement, and the fine-tune driver on the HIP backend: the
reference trajectory fixture, the four single-step fixtures with FusedCrossEntropy as the criterion, graph capture, host reads,
and `python -m rspnet_amd.finetune` end to end on SyntheticLabelledClips."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 2e-5      # the project's per-kernel gate, relative L2 against fp64
CLASSES = (1, 4, 5, 11, 51, 101, 174, 400, 1000, 4096)
N_CROPS = (1, 2, 3, 10)


def dev():
    return torch.device("cuda", 0)


# Where check_case places its operands on the device.  tests/test_guarded_downstream_gpu.py runs it with these two pointed at guarded
# allocations (tests/guarded.py): place() for inputs, place_empty() for what the kernel updates in place.
def place(t):
    return t.to(dev())


def place_empty(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=dev())


def restate(logits, n_crop, target, valid):
    """fp64 restatement of rsp_xent_metrics.  The crop mean is DEFINED in fp32 (sum in crop order, one division), so the ranks are
    taken on that fp32 mean, evaluated here with numpy's fp32 arithmetic; everything else is fp64."""
    rows, classes = logits.shape
    S = rows // n_crop
    x = logits.reshape(S, n_crop, classes)
    avg32 = np.zeros((S, classes), dtype=np.float32)
    for j in range(n_crop):
        avg32 = (avg32 + x[:, j]).astype(np.float32)
    if n_crop > 1:
        avg32 = (avg32 / np.float32(n_crop)).astype(np.float32)
    avg = x.astype(np.float64).mean(axis=1)
    m = avg.max(axis=1, keepdims=True)
    lse = np.log(np.exp(avg - m).sum(axis=1)) + m[:, 0]
    loss_s = lse - avg[np.arange(S), target]
    p = np.exp(avg - lse[:, None])
    p[np.arange(S), target] -= 1.0
    dlogits = np.repeat(p / (S * n_crop), n_crop, axis=0)
    vt = avg32[np.arange(S), target][:, None]
    rank = ((avg32 > vt) | ((avg32 == vt) & (np.arange(classes)[None] < target[:, None]))).sum(axis=1)
    h1, h5 = int((rank[:valid] == 0).sum()), int((rank[:valid] < 5).sum())
    return avg, float(loss_s.mean()), dlogits, h1, h5


def l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def acc_of(hits, valid):
    return float(np.float32(hits) * np.float32(100.0 / valid))


def read_meters(buf):
    h = buf.cpu().numpy()
    return h[0:12].view(np.float32).copy(), h[12:24].view(np.float32).copy(), h[24:36].view(np.int32).copy()


def check_case(be, logits, n_crop, target, valid, padded=False):
    rows, classes = logits.shape
    if padded:      # ld > classes: a column slice of a wider matrix
        wide = torch.full((rows, classes + 3), float("nan"))
        wide[:, :classes] = torch.from_numpy(logits)
        lt = place(wide)[:, :classes]
    else:
        lt = place(torch.from_numpy(logits))
    meters = place_empty(36, dtype=torch.uint8).zero_()
    avg, loss, acc, dl = be.xent_metrics(lt, place(torch.from_numpy(target)), n_crop=n_crop, valid=valid, meters=meters)
    ravg, rloss, rdl, h1, h5 = restate(logits, n_crop, target, valid)
    assert l2(avg.cpu().numpy(), ravg) <= GATE
    assert abs(float(loss) - rloss) <= GATE * max(abs(rloss), 1e-30) or rloss == 0.0 == float(loss), (float(loss), rloss)
    assert l2(dl.cpu().numpy(), rdl) <= GATE or float(np.abs(rdl).max()) == 0.0 == float(dl.abs().max())
    val, total, count = read_meters(meters)
    if valid == 0:
        assert count.tolist() == [0, 0, 0] and total.tolist() == [0, 0, 0]
        return
    a = acc.cpu().numpy()
    assert a[0] == acc_of(h1, valid), (a, h1, valid)
    if classes >= 5:
        assert a[1] == acc_of(h5, valid), (a, h5, valid)
        assert count.tolist() == [valid] * 3 and val[2] == a[1]
    else:
        assert count.tolist() == [valid, valid, 0] and total[2] == 0.0 and val[2] == 0.0
    assert val[0] == float(loss) and val[1] == a[0]
    assert total[0] == np.float32(np.float32(float(loss)) * np.float32(valid))


def test_kernel_sweep_against_fp64():
    from rspnet_amd import ops
    be = ops.backend()
    assert be.name == "hip"
    rng = np.random.default_rng(11)
    n = 0
    for classes in CLASSES:
        for n_crop in N_CROPS:
            all_rows = [r for r in range(1, 81) if r % n_crop == 0]
            rows_list = all_rows if classes <= 101 and n_crop == 1 else sorted({all_rows[0], all_rows[len(all_rows) // 3], all_rows[-1]})
            for rows in rows_list:
                S = rows // n_crop
                scale = 80.0 if (rows + classes) % 3 == 0 else 1.0      # +-80: the row max must be subtracted first
                logits = (rng.uniform(-1, 1, (rows, classes)) * scale).astype(np.float32)
                target = rng.integers(0, classes, S).astype(np.int64)
                for valid in sorted({0, 1, S // 2, S}):
                    check_case(be, logits, n_crop, target, valid, padded=(n % 2 == 1))
                    n += 1
    print(f"\n{n} cases")


def test_constructed_ties_and_boundaries():
    from rspnet_amd import ops
    be = ops.backend()
    # integer logits: every tie is exact, also after the crop mean (n_crop = 2, both crops equal)
    rng = np.random.default_rng(3)
    logits = rng.integers(0, 3, (40, 9)).astype(np.float32).repeat(2, axis=0)
    target = rng.integers(0, 9, 40).astype(np.int64)
    check_case(be, logits, 2, target, 40)
    check_case(be, logits, 2, target, 17)
    flat = np.ones((6, 7), dtype=np.float32)
    t = np.array([0, 1, 4, 5, 6, 3], dtype=np.int64)
    avg, loss, acc, _ = be.xent_metrics(torch.from_numpy(flat).to(dev()), torch.from_numpy(t).to(dev()))
    assert acc.tolist() == [acc_of(1, 6), acc_of(4, 6)]      # ranks 0, 1, 4, 5, 6, 3: the lower class index wins a tie
    assert abs(float(loss) - np.log(7.0)) < 1e-6


def test_bad_targets_and_nan_logits_have_a_defined_result():
    """Rows chosen so that nothing faults: a target outside [0, classes) is never used as an index."""
    from rspnet_amd import _lib, ops
    be = ops.backend()
    logits = np.zeros((5, 6), dtype=np.float32)
    logits[np.arange(5), [0, 1, 2, 3, 4]] = 4.0
    good = np.array([0, 1, 2, 3, 4], dtype=np.int64)
    for bad_t in (6, -1, 1 << 40):
        t = good.copy()
        t[2] = bad_t
        meters = torch.zeros(36, dtype=torch.uint8, device=dev())
        avg, loss, acc, dl = be.xent_metrics(torch.from_numpy(logits).to(dev()), torch.from_numpy(t).to(dev()), meters=meters)
        assert np.isnan(float(loss)) and acc.tolist() == [acc_of(4, 5), acc_of(4, 5)]
        assert torch.equal(avg.cpu(), torch.from_numpy(logits))
        assert bool(dl[2].isnan().all()) and bool(dl[[0, 1, 3, 4]].isfinite().all())
        assert read_meters(meters)[2].tolist() == [5, 5, 5]
    x = logits.copy()
    x[1, 5] = np.nan
    avg, loss, acc, dl = be.xent_metrics(torch.from_numpy(x).to(dev()), torch.from_numpy(good).to(dev()))
    assert np.isnan(float(loss)) and acc.tolist() == [acc_of(4, 5), acc_of(4, 5)]
    # outside the implemented ranges: an error with text, nothing launched
    big = torch.zeros((2, 4097), device=dev())
    with pytest.raises(_lib.RspError, match="classes"):
        be.xent_metrics(big, torch.zeros(2, dtype=torch.int64, device=dev()))
    with pytest.raises(_lib.RspError):
        be.xent_metrics(torch.zeros((6, 4), device=dev()), torch.zeros(2, dtype=torch.int64, device=dev()), n_crop=4)
    lib = be.lib
    z = torch.zeros((6, 4), device=dev())
    tz = torch.zeros(2, dtype=torch.int64, device=dev())
    out = torch.zeros(64, device=dev())
    rc = lib.rsp_xent_metrics(z.data_ptr(), 6, 4, 4, 4, tz.data_ptr(), 1, out.data_ptr(), None, out.data_ptr(), out.data_ptr(), None,
                              out.data_ptr(), 256, None)
    assert rc == -1 and b"n_crop" in lib.rsp_last_error()
    rc = lib.rsp_xent_metrics(z.data_ptr(), 6, 4, 4, 3, tz.data_ptr(), 3, out.data_ptr(), None, out.data_ptr(), out.data_ptr(), None,
                              out.data_ptr(), 256, None)
    assert rc == -1 and b"valid" in lib.rsp_last_error()


def test_determinism_and_meter_accumulation():
    from rspnet_amd import ops
    be = ops.backend()
    rng = np.random.default_rng(5)
    meters = torch.zeros(36, dtype=torch.uint8, device=dev())
    total = np.zeros(3, dtype=np.float32)
    count = 0
    for call in range(6):
        S, n_crop, classes = 7 + call, 2, 101
        lt = torch.from_numpy(rng.normal(size=(S * n_crop, classes)).astype(np.float32)).to(dev())
        tt = torch.from_numpy(rng.integers(0, classes, S)).to(dev())
        valid = S - call % 3
        a = be.xent_metrics(lt, tt, n_crop=n_crop, valid=valid, meters=meters)
        b = be.xent_metrics(lt, tt, n_crop=n_crop, valid=valid)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        single = torch.zeros(36, dtype=torch.uint8, device=dev())
        be.xent_metrics(lt, tt, n_crop=n_crop, valid=valid, meters=single)
        val1, sum1, count1 = read_meters(single)
        total = (total + sum1).astype(np.float32)      # N single-call contributions accumulated in fp32, in call order
        count += valid
        val, msum, mcount = read_meters(meters)
        assert np.array_equal(msum, total) and mcount.tolist() == [count] * 3 and np.array_equal(val, val1)


def test_graph_capture_and_replay():
    from rspnet_amd import ops
    be = ops.backend()
    rng = np.random.default_rng(9)
    S, n_crop, classes, valid = 8, 2, 51, 6
    lt = torch.from_numpy(rng.normal(size=(S * n_crop, classes)).astype(np.float32)).to(dev())
    tt = torch.from_numpy(rng.integers(0, classes, S)).to(dev())
    meters = torch.zeros(36, dtype=torch.uint8, device=dev())
    eager = be.xent_metrics(lt, tt, n_crop=n_crop, valid=valid, meters=meters)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = be.xent_metrics(lt, tt, n_crop=n_crop, valid=valid, meters=meters)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    val, total, count = read_meters(meters)
    assert count.tolist() == [4 * valid] * 3
    for u, v in zip(eager, cap):
        assert torch.equal(u, v)
    assert val[0] == float(eager[1])


@pytest.mark.parametrize("arch", ["c3d", "resnet18", "r2plus1d-vcop", "s3dg"])
def test_fused_criterion_on_the_single_step_fixtures(arch, monkeypatch):
    """finetune_util.check_case with FusedCrossEntropy in place of nn.CrossEntropyLoss: the same loss and gradient gates."""
    import finetune_util as F
    from rspnet_amd.finetune import FusedCrossEntropy
    made = []

    def factory(*a, **k):
        made.append(FusedCrossEntropy())
        return made[-1]

    monkeypatch.setattr(torch.nn, "CrossEntropyLoss", factory)
    worst = F.check_case(arch, dev(), 1e-3)
    assert len(made) == 1 and made[0].output is not None
    print(f"\n{arch}: worst gradient summary error with the fused criterion {worst:.2e}")


def test_engine_loop_matches_the_reference_trajectory(tmp_path):
    import finetune_loop_util as U
    from rspnet_amd import ops
    assert ops.backend().name == "hip"
    U.run_and_compare(tmp_path, U.fwd_tol("c3d", 2e-4))


def test_no_host_read_between_log_lines(tmp_path, monkeypatch):
    """Meters.read is the only host synchronisation of the loop: with log_interval = 2 over 3 train steps and 2 validate steps it
    runs once at the log line of iteration 2 and once at the end of each epoch context."""
    import finetune_loop_util as U
    from rspnet_amd import finetune
    z, meta, state = U.load()
    eng = U.build_engine(meta, state, tmp_path)
    reads = []
    orig = finetune.Meters.read
    monkeypatch.setattr(finetune.Meters, "read", lambda self: (reads.append(1), orig(self))[1])
    eng.train_epoch()
    assert len(reads) == 2      # the log line before iteration 2, the epoch summary
    eng.validate_epoch()
    assert len(reads) == 3      # 2 iterations: no log line (i = 1 is not a multiple of 2), the epoch summary


def run_cli(argv, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "rspnet_amd.finetune"] + argv, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    return r


FINAL = re.compile(r"Validation finished\.\n\tLoss = (\S+)\n\tAcc@1 = (\S+)% \((\d+)/(\d+)\)\n\tAcc@5 = (\S+)% \((\d+)/(\d+)\)")


def test_end_to_end_command_line(tmp_path):
    """python -m rspnet_amd.finetune on SyntheticLabelledClips, small sizes: trains (three epochs; `-d` caps a run at ONE epoch, as
    in the reference, so the training run goes without it and the validate-only run carries it), writes the run files, learns the
    synthetic classes, and a second process reproduces the final validation digit for digit."""
    exp, run1, run2 = tmp_path / "exp", tmp_path / "exp" / "run_a", tmp_path / "exp" / "run_b"
    classes = 5
    small = json.dumps({"dataset": {"num_classes": classes}, "batch_size": 8, "validate": {"batch_size": 8},
                        "final_validate": {"batch_size": 4}, "num_epochs": 3, "log_interval": 4,
                        "optimizer": {"lr": 0.01, "schedule": "cosine"}, "spatial_transforms": {"size": 32},
                        "temporal_transforms": {"size": 16, "validate": {"n_crop": 1, "final_n_crop": 3}}})
    cfg = os.path.join(ROOT, "rspnet_amd", "config", "finetune", "c3d.json")
    base = ["-c", cfg, "-x", small, "-e", str(exp), "--steps-per-epoch", "12", "--val-samples", "30", "--seed", "3"]
    r = run_cli(base + ["--run-dir", str(run1)], 420)
    assert r.returncode == 0, r.stderr[-3000:]
    for f in ("checkpoint.pth.tar", "model_best.pth.tar"):
        assert (exp / f).exists(), f
    for f in ("config.json", "run.sh", "experiment.log", "scalars.jsonl"):
        assert (run1 / f).exists(), f
    scalars = [json.loads(l) for l in open(run1 / "scalars.jsonl")]
    assert len(scalars) == 3
    print("\ntrain loss per epoch", [s["train/loss"] for s in scalars], "val acc1", [s["val/acc1"] for s in scalars])
    assert scalars[-1]["train/loss"] < scalars[0]["train/loss"]
    finals = FINAL.findall(r.stderr)
    assert len(finals) == 4      # three epochs + the final multi-crop validation
    print("final validation:", finals[-1])
    assert float(finals[-1][1]) > 100.0 / classes and int(finals[-1][3]) == 30
    r2 = run_cli(base + ["--run-dir", str(run2), "-d", "--validate", "--load-checkpoint", str(exp / "model_best.pth.tar")], 240)
    assert r2.returncode == 0, r2.stderr[-3000:]
    again = FINAL.findall(r2.stderr)
    assert len(again) == 1 and again[0] == finals[-1], (again, finals[-1])
