"""GPU: what the search and metric kernels do with NaN and +-Inf, pinned to the rule include/rspnet_hip.h states.

Search (rsp_cosine_topk, rsp_knn_classify, rsp_topk_hits), Nq 70, Ng 300, D 66, k 7 and 200, 1 and 3 gallery splits.  Planted at the
borders of the 64-query block and of the 128-row gallery tiles (= the split borders at 3 splits): NaN, +Inf, -Inf (in the first k
chunk, the second, and the ragged last one) and a finite row whose squares overflow fp32.  The rule: a gallery row holding a NaN / Inf
is never returned and changes nothing else; a query row holding one gets -1 / +inf in every slot, no votes, pred 0, rank = its label;
an overflowing row behaves as a zero row.  Two assertions per case:
  * against the fp64 references of the value tests (fp64_topk of test_retrieval_gpu with its gap screening, knn_reference with the
    excuse rule of knn_util) on the inputs the rule describes: poisoned gallery rows removed, overflowing rows zeroed;
  * differentially: a second run on the gallery without the poisoned rows gives, index-mapped, the same bits for every query.

Metrics (rsp_xent_metrics, rsp_pretext_metrics): +-Inf logits at the target / the positive, at the row maximum and elsewhere, in
rows of a padded pitch, against F.cross_entropy (loss per sample, gradient) and torch.topk (accuracy) in float64."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import knn_util
import test_finetune_loop_gpu as X
import test_pretext_metrics_gpu as P
import test_retrieval_gpu as R
from rspnet_amd import knn, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN, INF, HUGE = float("nan"), float("inf"), 3.0e19      # HUGE^2 = 9e38 > FLT_MAX: one such element overflows the sum of squares
NQ, NG, D, NCLS, TEMP = 70, 300, 66, 10, 0.07
# row -> [(column, value)]: columns in the first 32-wide k chunk, the second, and the last (D = 66: columns 64, 65)
G_PLANT = {0: [(5, NAN)], 63: [(0, INF)], 64: [(33, -INF)], 127: [(7, -HUGE)], 128: [(65, NAN)], 299: [(1, INF), (40, -INF)]}
Q_PLANT = {0: [(64, NAN)], 63: [(31, INF)], 64: [(2, HUGE)], 69: [(32, -INF)]}
G_OVERFLOW, Q_OVERFLOW = [127], [64]
Q_LABELS = {0: 0, 63: 3, 69: 7}        # the labels of the non-finite queries: a "hit" at top-1, at top-5 only, a miss (rank = label)


@pytest.fixture(scope="module")
def be():
    assert ops.backend().name == "hip"
    return ops.backend()


@functools.lru_cache(maxsize=None)
def search_case():
    q, yq = knn_util.feats(701, NQ, D, NCLS, 0.5)
    g, yg = knn_util.feats(702, NG, D, NCLS, 0.5)
    for x, plant in ((q, Q_PLANT), (g, G_PLANT)):
        for row, marks in plant.items():
            for col, v in marks:
                x[row, col] = v
    for row, label in Q_LABELS.items():
        yq[row] = label
    bad_q = np.array(sorted(set(Q_PLANT) - set(Q_OVERFLOW)))
    bad_g = np.array(sorted(set(G_PLANT) - set(G_OVERFLOW)))
    assert not np.isfinite(q[bad_q]).all(axis=1).any() and not np.isfinite(g[bad_g]).all(axis=1).any()
    for x, rows in ((q, Q_OVERFLOW), (g, G_OVERFLOW)):
        with np.errstate(over="ignore"):
            assert np.isfinite(x[rows]).all() and np.isinf((x[rows] * x[rows]).sum(axis=1, dtype=np.float32)).all()
    clean_q = np.setdiff1d(np.arange(NQ), bad_q)
    keep_g = np.setdiff1d(np.arange(NG), bad_g)
    # the inputs as the rule sees them: an overflowing row is a zero row
    q_rule, g_rule = q.copy(), g.copy()
    q_rule[Q_OVERFLOW], g_rule[G_OVERFLOW] = 0, 0
    new_index = np.full(NG, -1, dtype=np.int64)
    new_index[keep_g] = np.arange(len(keep_g))
    out = dict(q=q, yq=yq, g=g, yg=yg, bad_q=bad_q, bad_g=bad_g, clean_q=clean_q, keep_g=keep_g, q_rule=q_rule[clean_q],
               g_rule=g_rule[keep_g], new_index=new_index)
    for a in out.values():
        a.setflags(write=False)
    return out


def to_dev(*arrays):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in arrays]


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check_lists(c, k, idx, dist):
    """idx / dist (device, all Nq rows) against the rule: the non-finite queries empty, no poisoned gallery row anywhere, the clean
    queries against fp64 on the rule's inputs (gap screening of test_retrieval_gpu), the overflowing query as a zero query."""
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.all(idx_h[c["bad_q"]] == -1) and np.all(dist_h[c["bad_q"]] == np.inf)
    assert not np.isin(idx_h, c["bad_g"]).any(), "a gallery row holding a NaN / Inf was returned"
    clean = idx_h[c["clean_q"]]
    assert clean.min() >= 0                                       # (k <= the rows left: every slot of a clean query is filled)
    mapped = torch.from_numpy(c["new_index"][clean])
    swapped, total = R.check_against_fp64(c["q_rule"], c["g_rule"], k, mapped, torch.from_numpy(dist_h[c["clean_q"]]))
    print(f"k={k}: {swapped} of {total} positions excused")
    assert swapped <= 0.5 * total
    for row in Q_OVERFLOW:
        assert idx_h[row].tolist() == c["keep_g"][:k].tolist() and np.all(dist_h[row] == 1.0)
    at_overflow = np.isin(idx_h, G_OVERFLOW)
    assert at_overflow.any() or k < 200                           # (similarity 0: about the middle of the 295 ranks)
    assert np.all(dist_h[at_overflow] == 1.0), "the overflowing gallery row is not at distance 1"


def map_back(c, idx2):
    keep = torch.from_numpy(c["keep_g"].copy()).to(idx2.device)
    return torch.where(idx2 >= 0, keep[idx2.clamp(min=0).long()].to(torch.int32), idx2)


@pytest.mark.parametrize("splits", [1, 3])
def test_cosine_topk_and_topk_hits(be, splits):
    c = search_case()
    k = 7
    q, g, yq, yg = to_dev(c["q"], c["g"], c["yq"], c["yg"])
    idx, dist = be.cosine_topk(q, g, k, splits=splits)
    check_lists(c, k, idx, dist)
    # differentially: the gallery without the poisoned rows
    keep = torch.from_numpy(c["keep_g"].copy()).to(DEV)
    idx2, dist2 = be.cosine_topk(q, g[keep].contiguous(), k, splits=splits)
    assert torch.equal(map_back(c, idx2), idx) and torch.equal(bits(dist2), bits(dist))
    # the other split count: the same bits
    idx3, dist3 = be.cosine_topk(q, g, k, splits=4 - splits)
    assert torch.equal(idx3, idx) and torch.equal(bits(dist3), bits(dist))
    # hit counts: the non-finite queries are counted for no k
    ks = [1, 5, 7]
    counts = be.topk_hits(idx, yq, yg, ks).cpu().tolist()
    idx_h = idx.cpu().numpy()
    want = [int(sum(c["yq"][r] in c["yg"][idx_h[r, :kk]] for r in c["clean_q"])) for kk in ks]
    assert counts == want and counts == be.topk_hits(map_back(c, idx2), yq, yg, ks).cpu().tolist()


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("k", [7, 200])
def test_knn_classify(be, k, splits):
    c = search_case()
    q, g, yq, yg = to_dev(c["q"], c["g"], c["yq"], c["yg"])
    res = be.knn_classify(q, g, yg, k, TEMP, NCLS, y_q=yq, want_idx=True, want_votes=True, splits=splits)
    check_lists(c, k, res.idx, res.dist)
    if k <= 64:
        idx, dist = be.cosine_topk(q, g, k, splits=splits)
        assert torch.equal(res.idx, idx) and torch.equal(bits(res.dist), bits(dist))
    # the non-finite queries: no neighbours, no votes, class 0, rank = the label
    bad = torch.from_numpy(c["bad_q"].copy()).to(DEV)
    assert bool((res.votes[bad] == 0).all()) and res.pred[bad].cpu().tolist() == [0] * len(c["bad_q"])
    assert res.rank[bad].cpu().tolist() == [Q_LABELS[int(r)] for r in c["bad_q"]]
    # the clean queries against fp64 on the rule's inputs
    cq = c["clean_q"]
    rank, votes, _, sim, nxt = knn.knn_reference(c["q_rule"], c["yq"][cq], c["g_rule"], c["yg"][c["keep_g"]], k, TEMP, NCLS)
    exc = knn_util.excused(c["yq"][cq], votes, sim, nxt, k)
    print(f"k={k} splits={splits}: {int(exc.sum())} of {len(cq)} clean queries excused")
    assert exc.sum() <= knn_util.CAP * len(cq) + 1
    got_rank, got_pred, got_votes = res.rank.cpu().numpy()[cq], res.pred.cpu().numpy()[cq], res.votes.cpu().numpy()[cq]
    assert np.array_equal(got_rank[~exc], rank[~exc]) and np.array_equal(got_pred[~exc], votes.argmax(axis=1)[~exc])
    knn_util.check_votes(got_votes, votes, ~exc)
    # hits: the ranks as they are, the non-finite queries included with rank = label
    all_rank = res.rank.cpu().numpy()
    assert res.hits.cpu().tolist() == [int((all_rank < 1).sum()), int((all_rank < 5).sum())]
    assert int((all_rank[c["bad_q"]] < 1).sum()) == 1 and int((all_rank[c["bad_q"]] < 5).sum()) == 2
    # differentially: the gallery without the poisoned rows, every output of every query
    keep = torch.from_numpy(c["keep_g"].copy()).to(DEV)
    res2 = be.knn_classify(q, g[keep].contiguous(), yg[keep].contiguous(), k, TEMP, NCLS, y_q=yq, want_idx=True, want_votes=True, splits=splits)
    assert torch.equal(map_back(c, res2.idx), res.idx) and torch.equal(bits(res2.dist), bits(res.dist))
    assert torch.equal(bits(res2.votes), bits(res.votes)) and torch.equal(res2.rank, res.rank)
    assert torch.equal(res2.pred, res.pred) and torch.equal(res2.hits, res.hits)
    # the other split count: the same bits
    res3 = be.knn_classify(q, g, yg, k, TEMP, NCLS, y_q=yq, want_idx=True, want_votes=True, splits=4 - splits)
    for a, b in zip(res3, res):
        assert torch.equal(bits(a), bits(b))


def test_fewer_clean_gallery_rows_than_k(be):
    """k = 200 over the first 130 gallery rows, five of them poisoned: 125 neighbours, then -1 / +inf."""
    c = search_case()
    q, g, yg = to_dev(c["q"], c["g"][:130], c["yg"][:130])
    res = be.knn_classify(q, g, yg, 200, TEMP, NCLS, want_idx=True, splits=2)
    idx_h, dist_h = res.idx.cpu().numpy(), res.dist.cpu().numpy()
    left = [r for r in range(130) if r not in c["bad_g"]]
    for row in c["clean_q"]:
        assert sorted(idx_h[row, :len(left)].tolist()) == left and np.all(idx_h[row, len(left):] == -1), row
        assert np.all(np.isfinite(dist_h[row, :len(left)])) and np.all(dist_h[row, len(left):] == np.inf)
    assert np.all(idx_h[c["bad_q"]] == -1)


# ---- rsp_xent_metrics --------------------------------------------------------------------------------------------------------
def _same_nonfinite_and_close(got, ref, what, rel=X.GATE):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{what}: NaNs in different places"
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf]), f"{what}: infinities differ"
    fin = torch.isfinite(ref)
    if bool(fin.any()):
        assert X.l2(got[fin].numpy(), ref[fin].numpy()) <= rel, what


@pytest.mark.parametrize("padded", [True, False], ids=["padded-pitch", "dense"])
@pytest.mark.parametrize("n_crop", [1, 2])
def test_xent_metrics_infinite_logits(be, n_crop, padded):
    """One sample per placement: +Inf / -Inf at the target, at the row maximum (off the target), elsewhere (the target third among
    the finite values: a top-5 hit only), two -Inf off the target, clean samples; with n_crop = 2 the Inf sits in one crop (the mean
    is Inf) and one more sample holds +Inf and -Inf in its two crops (the mean is NaN: a miss by the NaN rule).  Per sample the loss
    against F.cross_entropy in float64 (S = 1 calls), the batch gradient against autograd's, the accuracies against torch.topk."""
    classes, S = 11, 10 if n_crop == 2 else 9
    rng = np.random.default_rng(5 + n_crop)
    mean = rng.uniform(-2, 2, (S, classes)).astype(np.float32)
    target = rng.integers(0, classes, S)
    order = np.argsort(-mean, axis=1)
    for s in (2, 3):                                   # the row maximum off the target
        target[s] = order[s, 1]
    target[7] = order[7, 2]
    mean[0, target[0]] = INF
    mean[1, target[1]] = -INF
    mean[2, order[2, 0]] = INF
    mean[3, order[3, 0]] = -INF
    mean[6, [c for c in range(classes) if c != target[6]][:2]] = -INF
    mean[7, order[7, 5]] = INF                         # +Inf off the target: the target is now third
    crops = np.repeat(mean[:, None], n_crop, axis=1)
    if n_crop == 2:
        fin = np.isfinite(mean)
        delta = rng.uniform(-0.5, 0.5, mean.shape).astype(np.float32)
        crops[:, 0][fin] += delta[fin]                 # the two crops differ; an Inf sits in crop 0 only
        crops[:, 1][fin] -= delta[fin]
        crops[:, 1][~fin] = 0.25
        crops[9, 0, 4], crops[9, 1, 4] = INF, -INF     # the crop mean of sample 9 is NaN
    logits = crops.reshape(S * n_crop, classes)
    avg32 = torch.from_numpy(crops).sum(dim=1) / n_crop if n_crop > 1 else torch.from_numpy(crops[:, 0])
    t = torch.from_numpy(target)

    def call(rows_logits, tgt, valid=None):
        lt = torch.from_numpy(rows_logits)
        if padded:
            wide = torch.full((lt.shape[0], classes + 3), NAN)
            wide[:, :classes] = lt
            lt = wide.to(DEV)[:, :classes]
        else:
            lt = lt.to(DEV)
        return be.xent_metrics(lt, tgt.to(DEV), n_crop=n_crop, valid=valid)

    avg, loss, acc, dl = call(logits, t)
    assert torch.equal(torch.isnan(avg.cpu()), torch.isnan(avg32)) and torch.equal(avg.cpu()[~torch.isnan(avg32)], avg32[~torch.isnan(avg32)])
    # float64 reference on the crop mean the kernel defines (fp32)
    x = avg32.double().requires_grad_(True)
    per_sample = F.cross_entropy(x, t, reduction="none")
    per_sample.mean().backward()
    assert torch.isnan(per_sample.mean()) and torch.isnan(loss.cpu()).all()
    want_dl = (x.grad / n_crop).repeat_interleave(n_crop, dim=0)
    _same_nonfinite_and_close(dl, want_dl, "dlogits")
    assert bool(torch.isnan(want_dl[0]).all()) and bool(torch.isfinite(want_dl[n_crop]).all())      # +Inf row: NaN; -Inf at the target: finite
    for s in range(S):                                 # the loss of every sample by itself
        _, loss_s, acc_s, _ = call(logits[s * n_crop:(s + 1) * n_crop], t[s:s + 1])
        _same_nonfinite_and_close(loss_s, per_sample[s:s + 1].detach(), f"loss of sample {s}")
    per_sample = per_sample.detach()
    assert float(per_sample[1]) == INF and torch.isnan(per_sample[[0, 2, 7]]).all() and torch.isfinite(per_sample[[3, 4, 5, 6, 8]]).all()
    # accuracy: torch.topk in float64 where no logit is NaN; a NaN mean is a miss
    has_nan = torch.isnan(avg32).any(dim=1)
    top = torch.topk(torch.nan_to_num(avg32.double(), nan=0.0), 5, dim=1).indices
    hit1 = (top[:, 0] == t) & ~has_nan
    hit5 = (top == t[:, None]).any(dim=1) & ~has_nan
    assert hit1.tolist()[:3] == [True, False, False] and hit5.tolist()[7] and not hit1.tolist()[7]
    for valid in (S, 5, 1):
        _, _, acc, _ = call(logits, t, valid)
        assert acc.cpu().tolist() == [X.acc_of(int(hit1[:valid].sum()), valid), X.acc_of(int(hit5[:valid].sum()), valid)], valid


# ---- rsp_pretext_metrics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K1", [65, 16385])
def test_pretext_metrics_infinite_logits(K1):
    """+-Inf at the positive and elsewhere (the scalar head, the float4 body and the last column of a 4-byte aligned row), +-Inf on
    either side of the ranking pair: the ranks, the restatement, and torch.topk in float64 (no row holds a NaN, no tie touches the
    positive)."""
    g = torch.Generator().manual_seed(K1)
    x = torch.randn(6, K1, generator=g) - 3.0
    x[:, 0] = 0.0                                      # finite positives: above every other column (at 16385 columns nearly every one)
    x[:, 1:] = x[:, 1:].clamp(max=-0.5)
    x[0, 0] = INF                                      # +Inf positive: rank 0
    x[1, 0] = -INF                                     # -Inf positive: every finite column stands ahead
    x[2, [7, K1 - 1]] = INF                            # two +Inf elsewhere: rank 2
    x[3, [1, 3, K1 - 2]] = -INF                        # -Inf elsewhere never counts: rank 0
    x[4, 0], x[4, 2], x[4, 40] = INF, -INF, -INF
    x[5, [1, 2, 3, 33, 40, K1 - 1]] = 1.0              # six finite columns above the positive: outside the top 5
    lp = torch.tensor([INF, -INF, 0.0, 0.0, 1.0, 0.0])
    ln = torch.tensor([0.0, 0.0, -INF, INF, 0.0, 1.0])
    acc, ranks = P.check(P.backend(), x, x.flip(0), lp, ln)
    want = [0, K1 - 1, 2, 0, 0, 6]
    assert ranks.tolist() == want + want[::-1]
    top = torch.topk(x.double(), 5, dim=1).indices
    h1, h5 = int((top[:, 0] == 0).sum()), int((top == 0).any(dim=1).sum())
    hm = int((torch.topk(torch.stack([lp, ln], dim=1).double(), 1, dim=1).indices[:, 0] == 0).sum())
    assert (h1, h5, hm) == (3, 4, 3)
    per = np.float32(100.0 / 6)
    assert acc.tolist() == [float(np.float32(h) * per) for h in (h1, h5, h1, h5, hm)]
