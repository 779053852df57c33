"""Generate tests/golden/finetune_loop_c3d.npz: a short fine-tune TRAJECTORY of the reference (build container only).
TEST INFRASTRUCTURE ONLY.

    python tools/gen_golden_finetune_loop.py

The model is the reference's MultiTaskWrapper(finetune=True) (oracle.ref_harness.build_reference_finetune); the loop body is
finetune.py:101-143 and :326-345 restated line by line below with the reference's own framework.metrics.classification.accuracy,
framework.meters.average.AverageMeter, nn.CrossEntropyLoss, torch.optim.SGD and MultiStepLR(milestones=[1]).

State and clips: portable (oracle.portable.fill_state / clips), C3D at 16 x 32 x 32, 11 classes, B = 4, with the guard band of
oracle/guard.py around the first step's ReLU decisions.  Trajectory: two epochs of three train steps, each followed by a validate
epoch with n_crop = 2 over 6 samples in batches of 4 -- the second batch wraps around to samples 0, 1 and is cut to 2 valid ones.

Recorded per step (10 steps): crop-averaged logits, loss, acc1 / acc5, the three meters' val / sum / count after the update, the
valid count; per epoch: LR, validate acc1, best_acc1; after the run: BatchNorm buffer summaries and the checkpoint's non-tensor
entries (optimizer param_groups, scheduler state).  The weights are not stored.

Drift floor: the same trajectory runs a second time in fp64 (model.double()); floor[t] = |loss32[t] - loss64[t]| / |loss64[t]|.

Seed screen (oracle-only, never a result of the code under test): on the fp64 run, at every recorded step and valid sample, with
the sample's logits sorted descending (v[0] >= v[1] ...), r the target's rank and R = v[0] - v[-1]:
    r == 0: v[0] - v[1] > 1e-3 R;  r == 1: v[0] - v[1] > 1e-3 R      (top-1 boundary)
    r == 4: v[4] - v[5] > 1e-3 R;  r == 5: v[4] - v[5] > 1e-3 R      (top-5 boundary)
    always: v[4] - v[5] > 1e-3 R                                      (positions 5 and 6)
and the fp32 and fp64 runs agree on every hit.  The first seed that passes is taken."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import guard
from oracle import portable as P
from oracle import ref_harness as R
from oracle import restatement as S

ARCH, B, T, HW, NCLS = "c3d", 4, 16, 32, 11
EPOCHS, TRAIN_STEPS, VAL_SAMPLES, N_CROP = 2, 3, 6, 2
SGD = {"lr": 0.01, "momentum": 0.9, "dampening": 0, "weight_decay": 1e-4, "nesterov": False}
MILESTONES = [1]
GAP = 1e-3
PATH = os.path.join(ROOT, "tests", "golden", "finetune_loop_c3d.npz")


def train_batch(seed, epoch, step):
    t = epoch * TRAIN_STEPS + step
    return P.clips(seed, 10 + t, (B, 3, T, HW, HW))[0], ((np.arange(B) * 3 + seed + t) % NCLS).astype(np.int64)


def val_set(seed):
    return P.clips(seed, 100, (VAL_SAMPLES, 3, N_CROP * T, HW, HW))[0], ((np.arange(VAL_SAMPLES) * 5 + seed) % NCLS).astype(np.int64)


def val_batches(seed):
    """Full batches; the tail repeats the first samples, as the distributed sampler pads (num_valid_samples = VAL_SAMPLES)."""
    x, y = val_set(seed)
    n = -(-VAL_SAMPLES // B)
    idx = np.arange(n * B) % VAL_SAMPLES
    return [(x[idx[b * B:(b + 1) * B]], y[idx[b * B:(b + 1) * B]]) for b in range(n)]


def initial_state(seed, spec):
    state = P.fill_state(spec, seed)
    x0 = train_batch(seed, 0, 0)[0]
    nudges, rep = guard.guard_band(ARCH, "linear", state, [x0], forward=lambda sd, xx: S.finetune_forward(ARCH, sd, xx, training=True))
    guard.apply_nudges(state, nudges)
    return state, nudges, rep


def reshape_clip(clip, n_crop):      # finetune.py:44-52 without the named-tensor spelling
    if n_crop == 1:
        return clip
    b, c, tt, h, w = clip.shape
    return clip.view(b, c, n_crop, tt // n_crop, h, w).permute(0, 2, 1, 3, 4, 5).reshape(b * n_crop, c, tt // n_crop, h, w)


def average_logits(logits, n_crop):      # finetune.py:54-61
    if n_crop == 1:
        return logits
    return logits.view(logits.size(0) // n_crop, n_crop, -1).mean(dim=1)


def run_trajectory(model, state, seed, dtype, max_steps=None):
    R._install_shims()
    from framework.meters.average import AverageMeter
    from framework.metrics.classification import accuracy
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    model = model.to(dtype)
    criterion = torch.nn.CrossEntropyLoss()
    optimizer = torch.optim.SGD(model.parameters(), **SGD)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer=optimizer, milestones=MILESTONES)
    rec = {k: [] for k in ("logits", "loss", "acc", "val", "sum", "count", "valid", "train", "target")}
    ep = {k: [] for k in ("lr", "val_acc1", "best_acc1")}
    best_acc1, current_epoch = 0., 0

    def forward(batches, n_crop, train):      # EpochContext.forward, finetune.py:95-146
        loss_meter, top1_meter, top5_meter = AverageMeter("Loss"), AverageMeter("Acc@1", fmt=":6.2f"), AverageMeter("Acc@5", fmt=":6.2f")
        remaining_valid_samples = VAL_SAMPLES if not train else len(batches) * B
        for i, (clip, target) in enumerate(batches):
            if max_steps is not None and len(rec["loss"]) >= max_steps:
                return
            clip, target = torch.from_numpy(clip).to(dtype), torch.from_numpy(target)
            clip = reshape_clip(clip, n_crop)
            output = model(clip)
            output = average_logits(output, n_crop)
            loss = criterion(output, target)
            full_output, full_target = output, target
            batch_size = target.size(0)
            if batch_size > remaining_valid_samples:
                output = output[:remaining_valid_samples]
                target = target[:remaining_valid_samples]
                batch_size = remaining_valid_samples
            remaining_valid_samples -= batch_size
            if batch_size == 0:
                continue
            acc1, acc5 = accuracy(output, target, topk=(1, 5))
            top1_meter.update(acc1, batch_size)
            top5_meter.update(acc5, batch_size)
            loss_meter.update(loss, batch_size)
            ms = (loss_meter, top1_meter, top5_meter)
            rec["logits"].append(full_output.detach().double().numpy().copy())
            rec["loss"].append(float(loss.detach()))
            rec["acc"].append([float(acc1), float(acc5)])
            rec["val"].append([float(m.val.detach()) for m in ms])
            rec["sum"].append([float(m.sum) for m in ms])
            rec["count"].append([int(m.count) for m in ms])
            rec["valid"].append(batch_size)
            rec["train"].append(int(train))
            rec["target"].append(full_target.numpy().copy())
            yield loss, top1_meter

    while current_epoch < EPOCHS:      # Engine.run, finetune.py:378-420
        ep["lr"].append(float(scheduler._last_lr[0]))
        model.train()
        for loss, _ in forward([train_batch(seed, current_epoch, s) for s in range(TRAIN_STEPS)], 1, True):
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        model.eval()
        top1 = None
        with torch.no_grad():
            for _, top1 in forward(val_batches(seed), N_CROP, False):
                pass
        if top1 is None:
            break
        acc1 = top1.avg.item()
        scheduler.step()
        current_epoch += 1
        best_acc1 = max(acc1, best_acc1)
        ep["val_acc1"].append(acc1)
        ep["best_acc1"].append(best_acc1)
    ckpt = {"epoch": current_epoch, "arch": ARCH, "best_acc1": best_acc1,
            "optimizer_param_groups": optimizer.state_dict()["param_groups"],
            "scheduler": {k: (dict(v) if hasattr(v, "items") else v) for k, v in scheduler.state_dict().items()}}
    post = {k: v.detach().double().numpy().copy() for k, v in model.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    return rec, ep, ckpt, post


def ranks(logits, target):
    vt = logits[np.arange(len(target)), target][:, None]
    cls = np.arange(logits.shape[1])[None]
    return ((logits > vt) | ((logits == vt) & (cls < target[:, None]))).sum(axis=1)


def well_separated(rec64):
    for logits, target, valid in zip(rec64["logits"], rec64["target"], rec64["valid"]):
        r = ranks(logits[:valid], target[:valid])
        for row, ri in zip(logits[:valid], r):
            v = np.sort(row)[::-1]
            thr = GAP * (v[0] - v[-1])
            if v[4] - v[5] <= thr or (ri in (0, 1) and v[0] - v[1] <= thr):
                return False
    return True


def main():
    torch.manual_seed(0)
    model = R.build_reference_finetune(ARCH, NCLS)
    spec = R.state_spec(model)
    for seed in range(3, 40):
        state, nudges, rep = initial_state(seed, spec)
        rec64, ep64, _, _ = run_trajectory(R.build_reference_finetune(ARCH, NCLS), state, seed, torch.float64)
        if not well_separated(rec64):
            print(f"seed {seed}: a rank boundary is closer than {GAP} of the logit range in fp64", flush=True)
            continue
        rec, ep, ckpt, post = run_trajectory(model, state, seed, torch.float32)
        if rec["acc"] != rec64["acc"]:
            print(f"seed {seed}: fp32 and fp64 reference runs disagree on a hit", flush=True)
            continue
        break
    else:
        raise SystemExit("no well-separated seed")
    loss32, loss64 = np.asarray(rec["loss"]), np.asarray(rec64["loss"])
    floor = np.abs(loss32 - loss64) / np.abs(loss64)
    meta = {"arch": ARCH, "B": B, "T": T, "HW": HW, "classes": NCLS, "seed": seed, "epochs": EPOCHS, "train_steps": TRAIN_STEPS,
            "val_samples": VAL_SAMPLES, "n_crop": N_CROP, "sgd": SGD, "milestones": MILESTONES, "checkpoint": ckpt,
            "spec": {k: [list(s), d] for k, (s, d) in spec.items()}}
    out = {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
           "logits": np.asarray(rec["logits"], dtype=np.float32), "loss": loss32, "loss64": loss64, "floor": floor,
           "acc": np.asarray(rec["acc"], dtype=np.float32), "meter_val": np.asarray(rec["val"], dtype=np.float32),
           "meter_sum": np.asarray(rec["sum"], dtype=np.float32), "meter_count": np.asarray(rec["count"], dtype=np.int32),
           "valid": np.asarray(rec["valid"], dtype=np.int32), "train": np.asarray(rec["train"], dtype=np.int32),
           "target": np.asarray(rec["target"], dtype=np.int64), "lr": np.asarray(ep["lr"]),
           "val_acc1": np.asarray(ep["val_acc1"]), "best_acc1": np.asarray(ep["best_acc1"])}
    for k, v in post.items():
        out["post." + k] = P.summarise(k, v) if v.ndim else np.asarray(v)
    for k, (idx, val) in (nudges or {}).items():
        out["nudge.idx." + k] = np.asarray(idx, dtype=np.int32)
        out["nudge.val." + k] = np.asarray(val, dtype=np.float32)
    np.savez_compressed(PATH, **out)
    print(f"seed {seed}: guard {rep}; losses {loss32.round(4).tolist()}; floor max {floor.max():.1e}; lr {ep['lr']}; "
          f"val acc1 {ep['val_acc1']}; {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
