"""Generate the retrieval fixtures under tests/golden/ from the REFERENCE's own retrieval.py (build container only).
TEST INFRASTRUCTURE ONLY.

    python tools/gen_golden_retrieval.py [features] [topk]

The live retrieval.py is imported after stubs for the modules this container lacks (pyhocon.config_tree, typed_args,
arguments, framework.config, torch.utils.tensorboard, torchvision, datasets.classification); the functions called are its
own: ``topk_retrieval`` and ``Engine.reshape_clip`` / ``Engine.average_clips`` (unbound, on a namespace holding n_crop).

retrieval_features_<arch>.npz: portable state (oracle.portable.fill_state, non-default BN running statistics) and portable clips
(B = 2, n_crop = 3, the fine-tune fixtures' sizes) through the reference pipeline: eval(), reshape_clip, get_feature,
AdaptiveAvgPool3d, squeeze, average_clips.  Stored: meta (seed, sizes, state spec), the features, the feature-map shape, and
the BN running buffers after one train-mode get_feature on the same crops.  Not the weights.

retrieval_topk.npz: class centroids plus noise from oracle.portable.uniform (600 gallery x 200 queries, D = 512, 20 classes;
drawn in a 6-dimensional latent space, see topk_inputs);
the reference's topk_correct and the fp64 top-50 indices / distances.  The seed is chosen on the fp64 distances alone (oracle-
only): every gap at a k boundary of KS >= 1e-5, every gap between neighbouring ranks of the top 50 >= 1e-6, and hit rates
strictly between 0 and 1 at every k."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import portable as P
from oracle import ref_harness as R

GOLDEN = os.path.join(ROOT, "tests", "golden")
# (arch, B, T, HW, classes, seed): the fine-tune fixtures' sizes (oracle/gen_golden_finetune.py)
FEATURE_CASES = [("c3d", 2, 16, 32, 11, 3), ("resnet18", 2, 16, 64, 11, 5), ("r2plus1d-vcop", 2, 16, 32, 11, 2),
                 ("s3dg", 2, 16, 64, 11, 7)]
N_CROP = 3
KS = (1, 5, 10, 20, 50)
NG, NQ, D, NCLS = 600, 200, 512, 20
LATENT = 6


def import_reference_retrieval():
    """The live /root/reference/retrieval.py with stubs for what this container lacks."""
    R._install_shims()

    def stub(name, **attrs):
        if name in sys.modules:
            return sys.modules[name]
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Any:
        def __init__(self, *a, **k):
            pass

    stub("pyhocon.config_tree", ConfigTree=sys.modules["pyhocon"].ConfigTree)
    import dataclasses
    stub("typed_args", TypedArgs=_Any, add_argument=lambda *a, **k: dataclasses.field(default=None))
    stub("arguments", Args=_Any)
    stub("framework.config", get_config=lambda *a, **k: None, save_config=lambda *a, **k: None)
    stub("torch.utils.tensorboard", SummaryWriter=_Any)
    stub("torchvision", transforms=types.SimpleNamespace())
    stub("datasets.classification", DataLoaderFactoryV3=_Any)
    import importlib
    return importlib.import_module("retrieval")


def reference_features(ret, arch, B, T, HW, ncls, seed):
    from models import get_model_class
    model = get_model_class(arch=arch)(num_classes=ncls)
    spec = R.state_spec(model)
    state = P.fill_state(spec, seed)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    x = P.clips(seed, 0, (B, 3, N_CROP * T, HW, HW))[0]
    ns = types.SimpleNamespace(n_crop=N_CROP)
    with torch.no_grad():
        model.eval()
        clip = ret.Engine.reshape_clip(ns, torch.from_numpy(x))
        fmap = model.get_feature(clip)
        out = torch.nn.AdaptiveAvgPool3d((1, 1, 1))(fmap).squeeze()
        feats = ret.Engine.average_clips(ns, out)
        model.train()
        model.get_feature(clip)
    post = {k: v.numpy().copy() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return spec, feats.numpy(), tuple(fmap.shape), post


def write_features(ret):
    for arch, B, T, HW, ncls, seed in FEATURE_CASES:
        spec, feats, fshape, post = reference_features(ret, arch, B, T, HW, ncls, seed)
        meta = {"arch": arch, "B": B, "T": T, "HW": HW, "classes": ncls, "seed": seed, "n_crop": N_CROP,
                "spec": {k: [list(s), d] for k, (s, d) in spec.items()}}
        out = {"meta": np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), "features": feats.astype(np.float32),
               "fmap_shape": np.asarray(fshape, dtype=np.int64)}
        out.update({"post:" + k: v.astype(np.float32) for k, v in post.items()})
        path = os.path.join(GOLDEN, f"retrieval_features_{arch.replace('-', '_')}.npz")
        np.savez_compressed(path, **out)
        print(f"{arch}: features {feats.shape}, map {fshape}, {os.path.getsize(path)} bytes")


def topk_inputs(seed):
    """Class centroids plus noise, all from oracle.portable, drawn in a LATENT space of LATENT dimensions and mapped to D by a
    portable basis: i.i.d. noise in 512 dimensions concentrates every cosine distance near 1, and the neighbouring-rank gaps of
    200 x 50 lists then fall below any usable separation."""
    cent = P.uniform("ret_centroid", seed, (NCLS, LATENT), -1.0, 1.0).astype(np.float64)
    basis = P.uniform("ret_basis", seed, (LATENT, D), -1.0, 1.0).astype(np.float64)
    yg = (P.permutation("ret_yg", seed, NG) % NCLS).astype(np.int64)
    yq = (P.permutation("ret_yq", seed, NQ) % NCLS).astype(np.int64)
    Xg = (cent[yg] + P.uniform("ret_xg", seed, (NG, LATENT), -1.0, 1.0)) @ basis
    Xq = (cent[yq] + P.uniform("ret_xq", seed, (NQ, LATENT), -1.0, 1.0)) @ basis
    return Xq.astype(np.float32), yq, Xg.astype(np.float32), yg


def fp64_topk(Xq, Xg, k):
    from sklearn.metrics.pairwise import cosine_distances
    d = cosine_distances(Xq.astype(np.float64), Xg.astype(np.float64))
    order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
    return order, np.take_along_axis(d, order, axis=1)


def well_separated(dist):
    gaps = np.diff(dist, axis=1)
    return min(float(gaps[:, k - 1].min()) for k in KS) >= 1e-5 and float(gaps[:, :max(KS)].min()) >= 1e-6


def reference_counts(ret, Xq, yq, Xg, yg, fold=1):
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, f"train_fold{fold}_feats.npy"), Xg.astype(np.float64))
        np.save(os.path.join(tmp, f"train_fold{fold}_labels.npy"), yg)
        np.save(os.path.join(tmp, f"test_fold{fold}_feats.npy"), Xq.astype(np.float64))
        np.save(os.path.join(tmp, f"test_fold{fold}_labels.npy"), yq)
        ret.topk_retrieval(tmp, sys.modules["pyhocon"].ConfigTree({"dataset.fold": fold}))
        with open(os.path.join(tmp, f"topk_correct_fold{fold}.json"), "rb") as f:
            raw = f.read()
    return {int(k): int(v) for k, v in json.loads(raw).items()}, raw


def write_topk(ret):
    for seed in range(1, 5000):
        Xq, yq, Xg, yg = topk_inputs(seed)
        order, dist = fp64_topk(Xq, Xg, max(KS))
        hits = [int((yg[order[:, :k]] == yq[:, None]).any(axis=1).sum()) for k in KS]
        if well_separated(dist) and all(0 < h < NQ for h in hits):
            break
    else:
        raise SystemExit("no well-separated seed")
    counts, raw = reference_counts(ret, Xq, yq, Xg, yg)
    assert all(0 < counts[k] < NQ for k in KS), counts
    meta = {"seed": seed, "NG": NG, "NQ": NQ, "D": D, "classes": NCLS, "ks": list(KS)}
    path = os.path.join(GOLDEN, "retrieval_topk.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8),
                        topk_correct=np.asarray([counts[k] for k in KS], dtype=np.int64),
                        json=np.frombuffer(raw, dtype=np.uint8), idx=order[:, :max(KS)].astype(np.int32),
                        dist=dist[:, :max(KS)])
    print(f"topk: seed {seed}, counts {counts}, {os.path.getsize(path)} bytes")


def main():
    torch.manual_seed(0)
    ret = import_reference_retrieval()
    only = sys.argv[1:]
    if not only or "features" in only:
        write_features(ret)
    if not only or "topk" in only:
        write_topk(ret)


if __name__ == "__main__":
    main()
