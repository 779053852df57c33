"""CPU: the fine-tune driver (rspnet_amd.finetune: Meters, FusedCrossEntropy on its torch composition, Engine, schedules,
checkpoints) on the torch checker backend, against the trajectory fixture generated from the reference
(tools/gen_golden_finetune_loop.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import finetune_loop_util as U
from cpu_ops import CpuOps
from golden_util import fwd_tol
from rspnet_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def cpu_backend():
    prev = ops.set_backend(CpuOps())
    yield
    ops.set_backend(prev)


def test_teacher_forced_criterion_and_meters(cpu_backend):
    """FusedCrossEntropy + Meters fed the recorded logits step by step: acc1 / acc5 and counts exact, loss and meter sums within
    1e-6 relative (fp32 rounding of an 11-term logsumexp).  Validate steps get each averaged row twice, as two equal crops."""
    from rspnet_amd.finetune import FusedCrossEntropy, Meters
    z, meta, _ = U.load()
    crit, meters = FusedCrossEntropy(), None
    for t in range(len(z["loss"])):
        if t == 0 or z["train"][t] != z["train"][t - 1]:
            meters = Meters("cpu")
        n_crop = 1 if z["train"][t] else meta["n_crop"]
        logits = torch.from_numpy(z["logits"][t]).repeat_interleave(n_crop, dim=0)
        loss = crit(logits, torch.from_numpy(z["target"][t]), n_crop=n_crop, valid=int(z["valid"][t]), meters=meters)
        assert torch.equal(crit.output, torch.from_numpy(z["logits"][t]))
        st = meters.read()
        assert [st[k]["count"] for k in meters.KEYS] == z["meter_count"][t].tolist()
        assert (st["acc1"]["val"], st["acc5"]["val"]) == tuple(float(a) for a in z["acc"][t])
        assert abs(float(loss) - z["loss"][t]) <= 1e-6 * abs(z["loss"][t])
        for i, k in enumerate(meters.KEYS):
            assert abs(st[k]["sum"] - z["meter_sum"][t][i]) <= 1e-6 * abs(z["meter_sum"][t][i]) + 0.0, (t, k)
            assert abs(st[k]["val"] - z["meter_val"][t][i]) <= 1e-6 * abs(z["meter_val"][t][i]), (t, k)
    pieces = meters.pieces()
    assert pieces[0] == "Loss {:f} ({:f})".format(st["loss"]["val"], st["loss"]["avg"])
    assert pieces[1] == "Acc@1 {:6.2f} ({:6.2f})".format(st["acc1"]["val"], st["acc1"]["avg"]) and pieces[2].startswith("Acc@5 ")
    assert str(meters) == "\t".join(pieces)
    meters.reset()
    assert meters.read()["loss"]["count"] == 0 and meters.read()["acc1"]["sum"] == 0.0
    meters.sync_distributed()      # no process group: a no-op


def test_valid_cut_small_class_count_and_ties(cpu_backend):
    from rspnet_amd.finetune import FusedCrossEntropy, Meters, rank_of_target
    crit, m = FusedCrossEntropy(), Meters("cpu")
    out = torch.tensor([[3., 1., 2., 0.], [0., 5., 1., 2.], [9., 0., 0., 0.], [0., 0., 0., 9.]], requires_grad=True)
    tgt = torch.tensor([0, 2, 1, 3])
    loss = crit(out, tgt, valid=3, meters=m)      # 4 classes: no acc5; the 4th sample is a repeat: not counted
    assert abs(float(loss.detach()) - float(torch.nn.functional.cross_entropy(out.detach(), tgt))) < 1e-6
    st = m.read()
    assert st["acc1"]["count"] == 3 and st["loss"]["count"] == 3 and st["acc5"]["count"] == 0 and st["acc5"]["sum"] == 0.0
    assert st["acc1"]["val"] == float(np.float32(1.0) * np.float32(100.0 / 3))      # only sample 0 hits (sample 2: tie rank 1)
    loss.backward()
    ref = torch.softmax(out.detach(), 1)
    ref[torch.arange(4), tgt] -= 1
    assert torch.allclose(out.grad, ref / 4, atol=1e-7)
    crit(out.detach(), tgt, valid=0, meters=m)      # nothing valid: meters untouched
    assert m.read()["loss"]["count"] == 3
    # exact ties go to the lower class index
    tie = torch.tensor([[1., 1., 1., 1., 1., 1., 1.]] * 3)
    assert rank_of_target(tie, torch.tensor([0, 4, 5])).tolist() == [0, 4, 5]
    m7 = Meters("cpu")
    crit(tie, torch.tensor([0, 4, 5]), meters=m7)
    st = m7.read()
    assert st["acc1"]["sum"] == pytest.approx(100.0) and st["acc5"]["sum"] == pytest.approx(200.0)
    with torch.no_grad():
        crit(out, tgt)
    assert crit.output.shape == (4, 4)


def test_engine_loop_matches_the_reference_trajectory(cpu_backend, tmp_path):
    U.run_and_compare(tmp_path, fwd_tol("c3d", 2e-4))
    ck = torch.load(tmp_path / "checkpoint.pth.tar", weights_only=False)
    assert list(ck) == ["epoch", "arch", "model", "best_acc1", "optimizer", "scheduler"]
    assert (tmp_path / "model_best.pth.tar").exists()
    lines = [json.loads(l) for l in open(tmp_path / "scalars.jsonl")]
    z = U.load()[0]
    assert [l["train/lr"] for l in lines] == z["lr"].tolist() and [l["epoch"] for l in lines] == [0, 1]
    assert set(lines[0]) == {"epoch", "train/lr", "train/loss", "train/acc1", "train/acc5", "val/loss", "val/acc1", "val/acc5"}


def test_checkpoint_interchange_and_continue(cpu_backend, tmp_path):
    """A checkpoint as the restated reference loop leaves it (its non-tensor entries travel in the fixture; the weights are the
    portable state) loads through Engine.load_checkpoint; ours has the reference's keys, and its optimizer / scheduler entries
    load into torch's own classes; --continue resumes at the saved epoch with the saved best_acc1."""
    z, meta, state = U.load()
    ck = meta["checkpoint"]
    sched = dict(ck["scheduler"])
    from collections import Counter
    sched["milestones"] = Counter({int(k): v for k, v in sched["milestones"].items()})
    ref_ckpt = {"epoch": ck["epoch"], "arch": ck["arch"], "model": {k: torch.from_numpy(v.copy()) for k, v in state.items()},
                "best_acc1": ck["best_acc1"], "optimizer": {"state": {}, "param_groups": ck["optimizer_param_groups"]},
                "scheduler": sched}
    torch.save(ref_ckpt, tmp_path / "ref.pth.tar")
    eng = U.build_engine(meta, state, tmp_path)
    eng.load_checkpoint(tmp_path / "ref.pth.tar")
    assert eng.current_epoch == 2 and eng.best_acc1 == float(z["best_acc1"][-1])
    assert eng.optimizer.param_groups[0]["lr"] == pytest.approx(0.001) and eng.scheduler.last_epoch == 2
    eng.run()      # epoch 2 of 2: nothing left to do
    assert not (tmp_path / "checkpoint.pth.tar").exists()
    bad = dict(ref_ckpt, arch="resnet18")
    torch.save(bad, tmp_path / "bad.pth.tar")
    with pytest.raises(ValueError, match="does not match"):
        eng.load_checkpoint(tmp_path / "bad.pth.tar")

    # ours -> torch's own classes
    eng = U.build_engine(meta, state, tmp_path)
    eng.num_epochs = 1
    eng.run()
    mine = torch.load(tmp_path / "checkpoint.pth.tar", weights_only=False)
    assert list(mine) == list(ref_ckpt) and mine["epoch"] == 1 and mine["arch"] == "c3d"
    assert list(mine["model"]) == list(state)
    params = [torch.nn.Parameter(torch.zeros_like(p)) for p in eng.model.parameters()]
    opt = torch.optim.SGD(params, lr=1.0, momentum=0.9)
    opt.load_state_dict(mine["optimizer"])
    assert opt.param_groups[0]["lr"] == 0.001 and opt.param_groups[0]["weight_decay"] == 1e-4
    assert len(opt.state) == sum(p.grad is not None for p in eng.model.parameters()) > 30      # momentum buffers came along
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[7])
    sch.load_state_dict(mine["scheduler"])
    assert sch.last_epoch == 1 and dict(sch.milestones) == {1: 1}

    # --continue: previous run's config + EXP/checkpoint.pth.tar (the helpers of rspnet_amd.pretrain)
    from rspnet_amd import finetune
    run0 = tmp_path / "run_0_x"
    run0.mkdir()
    with open(run0 / "config.json", "w") as f:
        json.dump(U.config(meta), f)
    args = finetune.parse_args(["-e", str(tmp_path), "--continue"])
    assert args.config == str(run0 / "config.json") and args.load_checkpoint == str(tmp_path / "checkpoint.pth.tar")
    assert os.path.basename(args.run_dir).startswith("run_1_")
    eng = U.build_engine(meta, state, tmp_path)
    eng.load_checkpoint(args.load_checkpoint)
    assert eng.current_epoch == 1 and eng.best_acc1 == mine["best_acc1"]


@pytest.mark.parametrize("schedule", ["plateau", "multi_step", "cosine", "none"])
def test_schedules_follow_torch(schedule):
    from rspnet_amd.finetune import build_scheduler
    cfg = {"optimizer": {"patience": 1, "milestones": [2, 4]}}

    def make():
        return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, momentum=0.9)

    losses = [1.0, 1.1, 1.2, 1.3, 1.4]
    mine_opt, ref_opt = make(), make()
    mine = build_scheduler(schedule, mine_opt, cfg, 5, 0.1)
    S = torch.optim.lr_scheduler
    ref = {"plateau": lambda: S.ReduceLROnPlateau(ref_opt, mode="min", patience=1),
           "multi_step": lambda: S.MultiStepLR(ref_opt, milestones=[2, 4]),
           "cosine": lambda: S.CosineAnnealingLR(ref_opt, T_max=5, eta_min=0.1 / 1000),
           "none": lambda: S.LambdaLR(ref_opt, lr_lambda=lambda e: 1)}[schedule]()
    assert type(mine) is type(ref)
    seq = []
    for e in range(5):
        seq.append((mine_opt.param_groups[0]["lr"], ref_opt.param_groups[0]["lr"]))
        for o in (mine_opt, ref_opt):
            o.step()
        if schedule == "plateau":
            mine.step(losses[e])
            ref.step(losses[e])
        else:
            mine.step()
            ref.step()
    assert [a for a, _ in seq] == [b for _, b in seq]
    assert len({a for a, _ in seq}) > 1 or schedule == "none"
    torch.save(mine.state_dict(), os.devnull)      # every schedule's state can be checkpointed


def test_unknown_schedule_and_1stream_raise(cpu_backend, tmp_path):
    from rspnet_amd.finetune import Engine, build_scheduler
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    with pytest.raises(ValueError):
        build_scheduler("step", opt, {}, 5, 0.1)
    z, meta, _ = U.load()
    cfg = dict(U.config(meta), model_type="1stream")
    with pytest.raises(NotImplementedError, match="1stream"):
        Engine(U.make_args(tmp_path), cfg, 0, train_loader=[], validate_loader=[])
    with pytest.raises(ValueError, match="model_type"):
        Engine(U.make_args(tmp_path), dict(cfg, model_type="2stream"), 0, train_loader=[], validate_loader=[])


def test_plateau_steps_on_the_last_train_loss(cpu_backend, tmp_path, monkeypatch):
    z, meta, state = U.load()
    eng = U.build_engine(meta, state, tmp_path, schedule="plateau")
    seen = []
    cls = torch.optim.lr_scheduler.ReduceLROnPlateau
    orig = cls.step
    monkeypatch.setattr(cls, "step", lambda self, v, *a, **k: (seen.append(v), orig(self, v, *a, **k))[1])
    eng.num_epochs = 1
    eng.run()
    assert seen == [eng.train_stats["loss"]["val"]] and abs(seen[0] - float(z["loss"][2])) <= 1e-3 * float(z["loss"][2])


def test_shipped_configs_hold_what_the_driver_reads():
    from rspnet_amd.finetune import _need
    cdir = os.path.join(ROOT, "rspnet_amd", "config", "finetune")
    names = sorted(os.listdir(cdir))
    assert names == ["c3d.json", "r2plus1d_vcop.json", "resnet18.json", "s3dg.json"]
    for n in names:
        with open(os.path.join(cdir, n)) as f:
            cfg = json.load(f)
        for key in ("model.arch", "model_type", "dataset.num_classes", "batch_size", "validate.batch_size", "final_validate.batch_size",
                    "num_epochs", "log_interval", "only_train_fc", "optimizer.lr", "optimizer.schedule", "spatial_transforms.size",
                    "temporal_transforms.size", "temporal_transforms.validate.n_crop", "temporal_transforms.validate.final_n_crop"):
            _need(cfg, key)


def test_synthetic_loader_protocol():
    from rspnet_amd.finetune import SyntheticLabelledClips
    tr = SyntheticLabelledClips("train", 10, 4, 5, 4, 8, "cpu", seed=1)
    va = SyntheticLabelledClips("val", 6, 4, 5, 4, 8, "cpu", n_crop=2, seed=1)
    assert len(tr) == 2 and tr.num_valid_samples() == 8 and len(va) == 2 and va.num_valid_samples() == 6 and va.dataset is va
    (clip,), target = next(iter(va))
    assert clip.shape == (4, 3, 8, 8, 8) and target.shape == (4,) and target.dtype == torch.int64
    batches = list(va)
    assert torch.equal(batches[1][0][0][2:], batches[0][0][0][:2]) and torch.equal(batches[1][1][2:], batches[0][1][:2])
    tr.set_epoch(0)
    a = [t for _, t in tr]
    tr.set_epoch(1)
    b = [t for _, t in tr]
    tr.set_epoch(0)
    assert all(torch.equal(x, y) for x, y in zip(a, [t for _, t in tr])) and next(iter(tr))[0][0].shape == (4, 3, 4, 8, 8)
    assert not all(torch.equal(x, y) for x, y in zip(a, b))


def test_fixture_first_step_against_the_live_reference():
    from oracle import ref_harness as R
    if not R.reference_available():
        pytest.skip("the reference tree is not on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_finetune_loop as G
    z, meta, state = U.load()
    rec, _, _, _ = G.run_trajectory(R.build_reference_finetune("c3d", meta["classes"]), state, meta["seed"], torch.float32, max_steps=1)
    from golden_util import rel_err
    assert rel_err(rec["logits"][0], z["logits"][0]) <= 1e-5      # (the host's thread count may move a convolution's sum order)
    assert abs(rec["loss"][0] - float(z["loss"][0])) <= 1e-5 and rec["acc"][0] == z["acc"][0].tolist()
    assert rec["count"][0] == z["meter_count"][0].tolist()
