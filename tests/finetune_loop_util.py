"""Shared by the fine-tune loop tests: the trajectory fixture tests/golden/finetune_loop_c3d.npz (tools/gen_golden_finetune_loop.py),
loaders over its portable clips, and the Engine run that is compared with it."""
import json
import os
import types

import numpy as np
import torch

from golden_util import fwd_tol, rel_err
from oracle import portable as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    z = np.load(os.path.join(GOLDEN, "finetune_loop_c3d.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    spec = {k: (tuple(s), d) for k, (s, d) in meta["spec"].items()}
    state = P.fill_state(spec, meta["seed"])
    for name in z.files:
        if name.startswith("nudge.idx."):      # the fixture's guard band (oracle/guard.py): part of its state
            key = name[len("nudge.idx."):]
            state[key][z[name].astype(np.int64)] = z["nudge.val." + key]
    return z, meta, state


def train_batch(meta, epoch, step):
    B, t = meta["B"], epoch * meta["train_steps"] + step
    x = P.clips(meta["seed"], 10 + t, (B, 3, meta["T"], meta["HW"], meta["HW"]))[0]
    return x, ((np.arange(B) * 3 + meta["seed"] + t) % meta["classes"]).astype(np.int64)


def val_set(meta):
    n = meta["val_samples"]
    x = P.clips(meta["seed"], 100, (n, 3, meta["n_crop"] * meta["T"], meta["HW"], meta["HW"]))[0]
    return x, ((np.arange(n) * 5 + meta["seed"]) % meta["classes"]).astype(np.int64)


class FixtureLoader:
    """The loader protocol of rspnet_amd.finetune.Engine over the fixture's clips.  train: the epoch's three batches; val: full
    batches whose tail wraps around to the first samples, num_valid_samples() = the real count."""

    def __init__(self, meta, split, device):
        self.meta, self.split, self.device, self.epoch, self.dataset = meta, split, device, 0, self
        if split == "val":
            x, y = val_set(meta)
            B, n = meta["B"], meta["val_samples"]
            idx = np.arange(-(-n // B) * B) % n
            self.val = [(torch.from_numpy(x[idx[b:b + B]]).to(device), torch.from_numpy(y[idx[b:b + B]]).to(device))
                        for b in range(0, len(idx), B)]

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.meta["train_steps"] if self.split == "train" else len(self.val)

    def num_valid_samples(self):
        return self.meta["train_steps"] * self.meta["B"] if self.split == "train" else self.meta["val_samples"]

    def __iter__(self):
        if self.split == "val":
            for x, y in self.val:
                yield (x,), y
        else:
            for s in range(self.meta["train_steps"]):
                x, y = train_batch(self.meta, self.epoch, s)
                yield (torch.from_numpy(x).to(self.device),), torch.from_numpy(y).to(self.device)


def config(meta, schedule="multi_step"):
    return {"model_type": "multitask", "model": {"arch": meta["arch"]}, "dataset": {"num_classes": meta["classes"]},
            "batch_size": meta["B"], "validate": {"batch_size": meta["B"]}, "final_validate": {"batch_size": meta["B"]},
            "num_epochs": meta["epochs"], "log_interval": 2, "only_train_fc": False,
            "optimizer": dict(meta["sgd"], type="sgd", schedule=schedule, milestones=meta["milestones"], patience=1, eps=1e-8),
            "spatial_transforms": {"size": meta["HW"]},
            "temporal_transforms": {"size": meta["T"], "validate": {"n_crop": meta["n_crop"], "final_n_crop": meta["n_crop"]}}}


def make_args(experiment_dir, **kw):
    return types.SimpleNamespace(experiment_dir=str(experiment_dir), run_dir=str(experiment_dir), debug=False, seed=0,
                                 steps_per_epoch=3, val_samples=6, **kw)


def build_engine(meta, state, experiment_dir, schedule="multi_step", final_validate=False):
    from rspnet_amd.finetune import Engine
    eng = Engine(make_args(experiment_dir), config(meta, schedule), 0, final_validate=final_validate,
                 train_loader=None if final_validate else FixtureLoader(meta, "train", _device()),
                 validate_loader=FixtureLoader(meta, "val", _device()))
    eng.model.module.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    return eng


def _device():
    return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")


def run_and_compare(experiment_dir, gate):
    """The whole Engine loop over the fixture's clips against the recorded trajectory.  gate: the forward tolerance of the
    project's fine-tune tests on this backend.  Exact: LR per epoch, meter counts, hits (acc1 / acc5), validate acc1, best_acc1.
    Step 0: logits and loss at `gate`.  Later steps: loss at max(gate, 3 * floor[t]), floor = the reference's own fp32 / fp64
    difference at that step (three-floor convention, the floor measured on the reference alone)."""
    z, meta, state = load()
    eng = build_engine(meta, state, experiment_dir)
    crit, steps = eng.criterion, []
    orig = crit.forward

    def recording(output, target, n_crop=1, valid=None, meters=None):
        loss = orig(output, target, n_crop=n_crop, valid=valid, meters=meters)
        steps.append((loss.detach().clone(), crit.output.clone(), meters.buf.clone()))
        return loss

    crit.forward = recording
    lrs = []
    orig_train = eng.train_epoch
    eng.train_epoch = lambda: (lrs.append(eng.optimizer.param_groups[0]["lr"]), orig_train())[1]
    eng.run()
    assert lrs == z["lr"].tolist()
    assert len(steps) == len(z["loss"])
    worst = {}
    for t, (loss, out, buf) in enumerate(steps):
        host = buf.cpu().numpy()
        val, total, count = host[0:12].view(np.float32), host[12:24].view(np.float32), host[24:36].view(np.int32)
        assert count.tolist() == z["meter_count"][t].tolist(), t
        # hits: the accuracies are hits * (100 / valid) on both sides, so equality is equality of the hit counts
        assert val[1] == z["acc"][t][0] and val[2] == z["acc"][t][1], (t, val, z["acc"][t])
        assert total[1] == z["meter_sum"][t][1] and total[2] == z["meter_sum"][t][2], t
        tol = gate if t == 0 else max(gate, 3.0 * float(z["floor"][t]))
        err = abs(float(loss) - float(z["loss"][t])) / max(1.0, abs(float(z["loss"][t])))
        print(f"step {t}: loss {float(loss):.6f} vs {float(z['loss'][t]):.6f} (err {err:.2e}, gate {tol:.2e})")
        worst[t] = err
        assert err <= tol, (t, err, tol)
        if t == 0:
            e = rel_err(out.cpu().numpy(), z["logits"][0])
            print(f"step 0: logits err {e:.2e}")
            assert e <= gate, e
    assert eng.validate_stats["acc1"]["avg"] == float(np.float32(z["val_acc1"][-1]))
    assert eng.best_acc1 == float(np.float32(z["best_acc1"][-1]))
    post = eng.model.module.state_dict()
    for name in z.files:
        if name.startswith("post."):
            k = name[5:]
            v = post[k].detach().cpu().numpy()
            if v.ndim == 0:
                assert int(v) == int(z[name]), k
            else:
                assert rel_err(P.summarise(k, v), z[name]) <= max(gate, 3.0 * float(z["floor"].max())), k
    return eng, worst


__all__ = ["load", "run_and_compare", "build_engine", "config", "make_args", "FixtureLoader", "fwd_tol"]
