"""Seeded inputs of the kNN classifier tests (CPU and GPU), their fp64 reference (computed once per case) and the excuse rule."""
import functools

import numpy as np

from rspnet_amd import knn

# (Nq, Ng, D, C, k, T, a)
CASES = [
    (1, 1, 2, 1, 1, 0.07, 1.0),                # smallest possible
    (9, 40, 66, 7, 64, 0.07, 0.5),             # Ng < k, D off the 32-wide chunk
    (33, 150, 2, 5, 200, 0.5, 1.0),            # Ng < k with four list slots, D = 2
    (130, 1000, 64, 10, 200, 0.07, 0.3),       # queries past one 64-row block
    (70, 300, 130, 101, 256, 0.07, 0.35),      # k at the limit
    (257, 2000, 512, 101, 200, 0.07, 0.15),    # several gallery tiles and splits
    (64, 2100, 32, 1024, 20, 0.07, 1.0),       # class limit, one list slot
]
SIM_GAP = 4e-6        # twice the 2e-6 similarity error tests/test_retrieval_gpu.py holds the search to
# votes: |ds| <= 2e-6 moves a weight by <= 2e-6 / T = 2.9e-5 relative at T = 0.07, an fp32 sum of <= 256 positive terms adds
# <= 256 * 2^-24 = 1.5e-5: 1e-4 of the query's largest vote covers both
VOTE_TOL = 1e-4
CAP = 0.05            # at most this share of a case's queries may be excused


def feats(seed, n, D, C, a):
    mu = np.random.default_rng(12345 + D + C).standard_normal((C, D))
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, n)
    x = (a * mu[y] + rng.standard_normal((n, D))).astype(np.float32)
    return x, y.astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    Nq, Ng, D, C, k, T, a = case
    q, yq = feats(Nq, Nq, D, C, a)
    g, yg = feats(Ng + 1, Ng, D, C, a)
    for arr in (q, yq, g, yg):
        arr.setflags(write=False)
    return q, yq, g, yg


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(rank, votes, topk_idx, topk_sim, next_sim, excused) in fp64; shared by the tests, read-only."""
    Nq, Ng, D, C, k, T, a = case
    q, yq, g, yg = case_inputs(case)
    rank, votes, idx, sim, nxt = knn.knn_reference(q, yq, g, yg, k, T, C)
    out = (rank, votes, idx, sim, nxt, excused(yq, votes, sim, nxt, min(k, Ng)))
    for arr in out:
        arr.setflags(write=False)
    return out


def excused(yq, votes, topk_sim, next_sim, kk):
    """From the reference alone: the k-th and (k+1)-th neighbour closer than SIM_GAP (the neighbour SET may differ), or the
    target's vote within 2 * VOTE_TOL relative (to the larger of the two) of another class's, both not zero (the RANK may differ)."""
    near_set = (topk_sim[:, kk - 1] - next_sim) < SIM_GAP
    C = votes.shape[1]
    good = (yq >= 0) & (yq < C)
    t = np.where(good, yq, 0)
    vt = votes[np.arange(len(yq)), t][:, None]
    other = np.arange(C)[None, :] != t[:, None]
    close = other & (votes != 0) & (vt != 0) & (np.abs(votes - vt) < 2 * VOTE_TOL * np.maximum(votes, vt))
    return near_set | (good & close.any(axis=1))


def check_votes(votes, ref_votes, keep):
    """votes (fp32, any array) against the fp64 reference on the rows `keep`: VOTE_TOL of each query's largest vote."""
    votes = np.asarray(votes, dtype=np.float64)
    scale = np.maximum(ref_votes.max(axis=1, keepdims=True), np.finfo(np.float64).tiny)
    err = np.abs(votes - ref_votes) / scale
    worst = float(err[keep].max()) if keep.any() else 0.0
    assert worst <= VOTE_TOL, worst
    return worst
