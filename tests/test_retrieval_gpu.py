"""GPU: the retrieval search kernels (rsp_cosine_topk / rsp_topk_hits) against an fp64 restatement, the backbones' get_feature
against the reference fixtures, and the retrieval pipeline end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from rspnet_amd import ops
from rspnet_amd import retrieval as ret

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = torch.device("cuda", 0)
GAP = 1e-5


# Where the test bodies place their operands on the device.  tests/test_guarded_memory_gpu.py runs the same bodies with these two
# pointed at guarded allocations (tests/guarded.py): dev() for inputs, dev_empty() for what a kernel writes.
def dev(t):
    return t.to(DEV)


def dev_empty(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=DEV)


def fp64_topk(q, g, k):
    """Restatement: sklearn's cosine_distances in fp64 (zero rows stay zero), ranked by distance, ties to the lower index."""
    q, g = q.astype(np.float64), g.astype(np.float64)
    nq, ng = np.linalg.norm(q, axis=1, keepdims=True), np.linalg.norm(g, axis=1, keepdims=True)
    qn, gn = q / np.where(nq == 0, 1, nq), g / np.where(ng == 0, 1, ng)
    d = np.clip(1.0 - qn @ gn.T, 0.0, 2.0)
    kk = min(k + 1, g.shape[0])
    part = np.argpartition(d, kk - 1, axis=1)[:, :kk] if kk < g.shape[0] else np.tile(np.arange(g.shape[0]), (q.shape[0], 1))
    pd = np.take_along_axis(d, part, axis=1)
    order = np.lexsort((part, pd), axis=1)
    return np.take_along_axis(part, order, axis=1), np.take_along_axis(pd, order, axis=1)


def features(seed, n, D, zero_rows=()):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, D)) + 0.5 * rng.standard_normal((1, D))).astype(np.float32)
    for r in zero_rows:
        x[r] = 0
    return x


def check_against_fp64(q, g, k, idx, dist):
    ridx, rd = fp64_topk(q, g, k)
    kk = min(k, g.shape[0])
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.all(idx[:, kk:] == -1) and np.all(np.isinf(dist[:, kk:]))
    assert float(np.abs(dist[:, :kk] - rd[:, :kk]).max()) <= 2e-6
    # positions whose fp64 neighbours (rank above / below, including rank k) are within GAP may legitimately swap
    gaps = np.diff(rd, axis=1)
    close = np.zeros((q.shape[0], kk), dtype=bool)
    close[:, 1:] |= gaps[:, :kk - 1] < GAP
    close[:, :kk] |= np.pad(gaps, ((0, 0), (0, 1)), constant_values=np.inf)[:, :kk] < GAP
    assert np.array_equal(idx[:, :kk][~close], ridx[:, :kk][~close])
    return int(close.sum()), close.size


SHAPES = [(1, 1, 512, 1), (7, 33, 512, 5), (119, 1000, 512, 50), (64, 5000, 1024, 50), (50, 3000, 2048, 64),
          (3783, 9537, 512, 50)]


@pytest.mark.parametrize("Nq,Ng,D,k", SHAPES)
def test_cosine_topk_matches_fp64(Nq, Ng, D, k):
    q, g = features(Nq, Nq, D), features(Ng + 1, Ng, D)
    idx, dist = ops.backend().cosine_topk(dev(torch.from_numpy(q)), dev(torch.from_numpy(g)), k)
    excused, total = check_against_fp64(q, g, k, idx, dist)
    print(f"({Nq},{Ng},{D},{k}): {excused} of {total} positions excused")
    assert excused <= 0.5 * total      # at least half of all positions are checked index for index


@pytest.mark.parametrize("Nq,Ng,D,k", [(5, 3, 64, 10), (9, 40, 66, 7), (70, 300, 130, 20), (33, 200, 2, 3)])
def test_cosine_topk_edges(Nq, Ng, D, k):
    """Ng < k (tail: -1 / +inf), D not a multiple of the 32-wide chunk, D = 2, query rows past a 64-row block."""
    q, g = features(1, Nq, D), features(2, Ng, D)
    idx, dist = ops.backend().cosine_topk(dev(torch.from_numpy(q)), dev(torch.from_numpy(g)), k)
    excused, total = check_against_fp64(q, g, k, idx, dist)
    assert excused <= 0.5 * total


def test_zero_rows_and_strided_inputs():
    q, g = features(3, 40, 512, zero_rows=(0, 17)), features(4, 700, 512, zero_rows=(3, 500))
    wide = dev_empty((40, 600)).zero_()
    wide[:, 8:520] = dev(torch.from_numpy(q))
    idx, dist = ops.backend().cosine_topk(wide[:, 8:520], dev(torch.from_numpy(g)), 20)
    check_against_fp64(q, g, 20, idx, dist)
    assert torch.equal(idx[0].cpu(), torch.arange(20, dtype=torch.int32)) and bool((dist[0] == 1).all())
    assert torch.equal(idx[17], idx[0])
    dz = dist.cpu().numpy()
    assert not np.any(idx.cpu().numpy()[1:17] == 3) or np.all(dz[idx.cpu().numpy() == 3] == 1)


def test_exact_ties_lower_index_first():
    g = features(5, 900, 512)
    for dup in (17, 300, 301, 640, 899):
        g[dup] = g[5]
    q = np.stack([g[5], g[5] * 2.0, g[100]])
    idx, dist = ops.backend().cosine_topk(dev(torch.from_numpy(q)), dev(torch.from_numpy(g)), 8, splits=4)
    idx = idx.cpu().numpy()
    assert list(idx[0, :6]) == [5, 17, 300, 301, 640, 899]
    assert list(idx[1, :6]) == [5, 17, 300, 301, 640, 899]
    assert idx[2, 0] == 100


def test_deterministic_across_runs_and_splits():
    lib = ops.backend().lib
    q, g = dev(torch.from_numpy(features(6, 300, 512))), dev(torch.from_numpy(features(7, 20000, 512)))
    g[1000:1010] = g[10]          # ties across split boundaries
    ref = ops.backend().cosine_topk(q, g, 50)
    used = {lib.rsp_cosine_topk_splits(300, 20000, s) for s in (0, 1, 3, 7, 16)}
    assert len(used) >= 4
    for s in (0, 1, 3, 7, 16):
        for _ in range(2):
            idx, dist = ops.backend().cosine_topk(q, g, 50, splits=s)
            assert torch.equal(idx, ref[0]) and torch.equal(dist.view(torch.int32), ref[1].view(torch.int32)), s


def test_no_nq_by_ng_allocation():
    Nq, Ng, D = 4096, 65536, 512
    q = dev_empty(Nq, D).copy_(torch.randn(Nq, D, device=DEV))
    g = dev_empty(Ng, D).copy_(torch.randn(Ng, D, device=DEV))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.max_memory_allocated(DEV)
    idx, dist = ops.backend().cosine_topk(q, g, 50)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak growth {grown / 2**20:.1f} MiB vs {Nq * Ng * 4 / 2**20:.0f} MiB for the matrix")
    assert grown < Nq * Ng * 4
    assert idx.shape == (Nq, 50)


def _topk_fixture():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_retrieval as gen
    z = np.load(os.path.join(GOLDEN, "retrieval_topk.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta, gen.topk_inputs(meta["seed"])


def test_topk_fixture_indices_and_json(tmp_path):
    z, meta, (Xq, yq, Xg, yg) = _topk_fixture()
    idx, dist = ops.backend().cosine_topk(dev(torch.from_numpy(Xq)), dev(torch.from_numpy(Xg)), 50)
    assert np.array_equal(idx.cpu().numpy(), z["idx"])
    assert float(np.abs(dist.cpu().numpy() - z["dist"]).max()) <= 2e-6
    for split, X, y in (("train", Xg, yg), ("test", Xq, yq)):
        np.save(tmp_path / f"{split}_fold1_feats.npy", X.astype(np.float64))
        np.save(tmp_path / f"{split}_fold1_labels.npy", y)
    counts = ret.topk_retrieval(str(tmp_path), 1)
    assert [counts[k] for k in meta["ks"]] == [int(c) for c in z["topk_correct"]]
    with open(tmp_path / "topk_correct_fold1.json", "rb") as f:
        assert f.read() == bytes(z["json"])


def test_topk_hits_counts():
    rng = np.random.default_rng(9)
    idx = rng.integers(-1, 50, (300, 20)).astype(np.int32)
    yq, yg = rng.integers(0, 7, 300), rng.integers(0, 7, 50)
    ks = [1, 3, 10, 20]
    counts = ops.backend().topk_hits(dev(torch.from_numpy(idx)), dev(torch.from_numpy(yq)), dev(torch.from_numpy(yg)), ks)
    want = [int(sum(any(j >= 0 and yg[j] == yq[r] for j in idx[r, :k]) for r in range(300))) for k in ks]
    assert counts.cpu().tolist() == want


# ---- get_feature -------------------------------------------------------------------------------------------------------
ARCHS = ["c3d", "resnet18", "r2plus1d_vcop", "s3dg"]


def _feature_case(arch):
    from oracle import portable as P
    from rspnet_amd.models import get_model_class
    z = np.load(os.path.join(GOLDEN, f"retrieval_features_{arch}.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    spec = {k: (tuple(s), d) for k, (s, d) in meta["spec"].items()}
    state = P.fill_state(spec, meta["seed"])
    model = get_model_class(arch=meta["arch"])(num_classes=meta["classes"])
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()})
    x = P.clips(meta["seed"], 0, (meta["B"], 3, meta["n_crop"] * meta["T"], meta["HW"], meta["HW"]))[0]
    return z, meta, model.to(DEV), dev(torch.from_numpy(x))


@pytest.mark.parametrize("arch", ARCHS)
def test_get_feature_eval_matches_reference(arch):
    from rspnet_amd.models import _SingleProcess
    z, meta, model, x = _feature_case(arch)
    eng = ret.Engine(_SingleProcess(model), n_crop=meta["n_crop"], device=DEV)
    model.eval()
    with torch.no_grad():
        fmap = model.get_feature(eng.reshape_clip(x))
        f = eng.features(x)
    assert tuple(fmap.shape) == tuple(int(s) for s in z["fmap_shape"])
    ref = z["features"]
    err = float(np.abs(f.cpu().numpy() - ref).max()) / float(np.abs(ref).max())
    print(f"{arch}: get_feature eval rel err {err:.2e}")
    assert f.shape == ref.shape and err <= 1e-4
    with pytest.raises(RuntimeError):
        model.get_feature(eng.reshape_clip(x))      # grad enabled on parameters that require grad: forward only


@pytest.mark.parametrize("arch", ARCHS)
def test_get_feature_train_mode_updates_running_stats(arch):
    z, meta, model, x = _feature_case(arch)
    from rspnet_amd.finetune import reshape_clip
    model.train()
    with torch.no_grad():
        model.get_feature(reshape_clip(x, meta["n_crop"]))
    sd = model.state_dict()
    worst = 0.0
    for key in z.files:
        if key.startswith("post:"):
            ref = z[key]
            mine = sd[key[5:]].cpu().numpy()
            worst = max(worst, float(np.abs(mine - ref).max()) / max(float(np.abs(ref).max()), 1e-12))
    print(f"{arch}: running-statistics rel err {worst:.2e}")
    assert worst <= 1e-4
    assert all(int(v) == int(meta["seed"]) % 5 + 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))


def test_get_feature_repacks_after_inplace_edit():
    z, meta, model, x = _feature_case("c3d")
    from rspnet_amd.finetune import reshape_clip
    from rspnet_amd.models import get_model_class
    clip = reshape_clip(x, meta["n_crop"])
    model.eval()
    with torch.no_grad():
        before = model.get_feature(clip).clone()
        model.conv3a.weight.mul_(0.5)
        after = model.get_feature(clip)
        fresh = get_model_class(arch="c3d")(num_classes=meta["classes"]).to(DEV)
        fresh.load_state_dict(model.state_dict())
        fresh.eval()
        want = fresh.get_feature(clip)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_retrieval_end_to_end(tmp_path):
    from model_util import make_cfg
    from rspnet_amd import finetune
    from rspnet_amd.framework.utils.checkpoint import CheckpointManager
    from rspnet_amd.models import ModelFactory, get_model_class
    from rspnet_amd.moco import ModelFactory as PretextFactory
    from rspnet_amd.moco.split_wrapper import MultiTaskWrapper
    torch.manual_seed(0)
    pre = PretextFactory(make_cfg("c3d", 64)).build_moco_diffloss(device=DEV).module
    CheckpointManager(str(tmp_path)).save({"epoch": 1, "arch": "c3d", "model": pre.state_dict()}, is_best=False, epoch=1)

    model = ModelFactory({"model": {"arch": "c3d"}, "dataset": {"num_classes": 101}}).build(0)
    n_crop = 2
    eng = ret.Engine(model, n_crop=n_crop, fold=1, device=DEV)
    eng.load_moco_checkpoint(str(tmp_path / "checkpoint.pth.tar"))
    def loader(nb, seed):
        r = np.random.default_rng(seed)
        return [((torch.from_numpy(r.standard_normal((2, 3, n_crop * 16, 32, 32)).astype(np.float32)),),
                 torch.from_numpy(r.integers(0, 3, 2))) for _ in range(nb)]
    train, test = loader(6, 1), loader(3, 2)
    feat_dir = str(tmp_path / "feature")
    eng.run(feat_dir, train, test)
    eng_b1 = ret.Engine(model, n_crop=n_crop, device=DEV)
    assert eng_b1.features(train[0][0][0][:1]).shape == (1, 512)      # batch of one stays (1, D)

    # features against MultiTaskWrapper(finetune=True).eval()'s pooled features on the same clips and weights
    mtw = MultiTaskWrapper(get_model_class(arch="c3d"), num_classes=101, finetune=True).to(DEV)
    mtw.encoder.load_state_dict({k: v for k, v in model.module.state_dict().items() if not k.startswith("linear.")}, strict=False)
    mtw.eval()
    Xtr, ytr, Xte, yte = ret.load_features(feat_dir, 1)
    with torch.no_grad():
        want = []
        for (clip,), _ in train:
            mtw(finetune.reshape_clip(dev(clip), n_crop))
            want.append(finetune.average_logits(ops.backend().spatial_mean_fwd(mtw.feat), n_crop).cpu().numpy())
    want = np.concatenate(want)
    assert Xtr.dtype == np.float64 and ytr.dtype == np.int64 and Xtr.shape == (12, 512)
    assert float(np.abs(Xtr - want).max()) <= 1e-5 * max(float(np.abs(want).max()), 1.0)

    ks = (1, 2, 5)
    counts = ret.topk_retrieval(feat_dir, 1, ks)
    ridx, _ = fp64_topk(Xte.astype(np.float32), Xtr.astype(np.float32), max(ks))
    expect = {k: int(sum(yte[r] in ytr[ridx[r, :k]] for r in range(len(yte)))) for k in ks}
    assert counts == expect
    with open(os.path.join(feat_dir, "topk_correct_fold1.json")) as f:
        assert json.load(f) == {str(k): v for k, v in expect.items()}
