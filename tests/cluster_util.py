"""Seeded inputs of the clustering tests (CPU and GPU), their fp64 references (computed once per case, read-only), the conditions the
cases were chosen for -- asserted from the fp64 reference alone, so a later change of generator cannot quietly void them -- and the
checks of one k-means iteration."""
import functools

import numpy as np

from knn_util import CAP, SIM_GAP, feats
from rspnet_amd import cluster

SIM_TOL = 2e-6            # what tests/test_retrieval_gpu.py holds the search's similarity to
A_STEP = 0.5
# (N, C, D): N in {1, 63, 64, 65, 129, 257} around the 64-row query block, C in {1, 2, 5, 101, 128, 129, 300, 1024} around the
# 128-row gallery tile and at the limit, D in {2, 30, 34, 200}; every value at least twice.  D = 2 is paired only with C <= 5: with
# C >= 101 centroids on the circle the fp64 reference alone has up to 45 % of its rows within SIM_GAP of a tie.
STEP_CASES = [(1, 1, 2), (257, 1, 200), (63, 2, 30), (129, 2, 2), (64, 5, 34), (65, 5, 2), (1, 101, 34), (129, 101, 200),
              (65, 128, 200), (64, 128, 30), (257, 129, 34), (63, 129, 30), (63, 300, 200), (129, 300, 34), (65, 1024, 30),
              (257, 1024, 200), (64, 2, 34), (129, 5, 30)]
# whole fits that must be reproduced exactly: (N, D, C, a, seed, iterations of the fp64 reference); init = x[default_rng(99 +
# seed).choice(N, C, replace=False)]; every best-to-second gap of every iteration is at least EXACT_GAP
EXACT_GAP = 1e-4          # 25 x SIM_GAP
EXACT_FITS = [(600, 34, 12, 2.0, 2, 6), (150, 2, 5, 1.0, 4, 12), (130, 66, 3, 1.0, 31, 6)]
# whole fits checked iteration by iteration from the reference's centroids: (N, D, C, a, max_iters); x = feats(N, ...), init =
# x[default_rng(99).choice(N, C, replace=False)]; the reference's own near-tie share stays below FORCED_SHARE in every iteration
FORCED_FITS = [(1000, 64, 10, 0.3, 20), (2100, 32, 256, 1.0, 10), (2000, 512, 101, 0.15, 15), (4000, 128, 16, 3.0, 20)]
FORCED_SHARE = 0.0015
EMPTY_CASE = (700, 64, 1024)      # N, D, C: the first 700 centroids are the rows, the rest random; 324 clusters stay empty


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def step_inputs(case):
    """(x, y, cent) of a one-iteration case: planted classes at a = 0.5, standard-normal centroids with a seed of their own."""
    N, C, D = case
    x, y = feats(1000 + N, N, D, C, A_STEP)
    cent = np.random.default_rng(777 + 31 * C + D).standard_normal((C, D)).astype(np.float32)
    return _freeze(x, y, cent)


def top_two(sim):
    """(best cluster, second cluster (-1 with one cluster), best similarity, gap) per row of an fp64 similarity matrix."""
    a, best, gap = cluster._assign_np(sim)
    rest = np.where(np.isnan(sim), -np.inf, sim).copy()
    rest[np.arange(sim.shape[0]), np.maximum(a, 0)] = -np.inf
    second = np.where(np.isfinite(rest.max(axis=1)), rest.argmax(axis=1), -1) if sim.shape[1] > 1 else np.full(sim.shape[0], -1)
    return a, second, best, gap


@functools.lru_cache(maxsize=None)
def step_reference(case):
    """(sim (N, C) fp64, assign, second, best, gap) of a one-iteration case."""
    x, _, cent = step_inputs(case)
    sim = cluster.reference_similarities(x, cent)
    return _freeze(sim, *top_two(sim))


def assert_step_conditions(case):
    """From the reference alone: D = 2 only with C <= 5, and no row of the case within SIM_GAP of a tie."""
    N, C, D = case
    assert D != 2 or C <= 5, case
    gap = step_reference(case)[4]
    assert float((gap < SIM_GAP).mean()) == 0.0, (case, float(gap.min()))


def check_iteration(x, cent_in, sim_ref, got_assign, got_sim, got_counts, got_cent, got_objective, what):
    """The checks of one iteration against the fp64 similarities ``sim_ref`` of (x, cent_in).  got_sim may be None.  Prints the figures
    before it asserts; returns them."""
    x = np.asarray(x, dtype=np.float32)
    N, C = sim_ref.shape
    a_ref, second, best, gap = top_two(sim_ref)
    got_assign = np.asarray(got_assign).astype(np.int64)
    excused = gap < SIM_GAP
    differs = got_assign != a_ref
    share = float(excused.mean())
    print(f"{what}: excused {int(excused.sum())}/{N}, differing {int(differs.sum())}, min gap {float(gap.min()):.3g}")
    assert share <= CAP, (what, share)
    assert not (differs & ~excused).any(), (what, np.nonzero(differs & ~excused)[0][:8])
    assert (~differs | (got_assign == second)).all(), what            # an excused row still takes one of the reference's top two
    got = got_assign >= 0
    mine = sim_ref[np.arange(N), np.maximum(got_assign, 0)]           # the reference similarity under the kernel's own assignment
    if got_sim is not None:
        err = float(np.abs(np.asarray(got_sim, dtype=np.float64)[got] - mine[got]).max()) if got.any() else 0.0
        print(f"{what}: sim error {err:.3g}")
        assert err <= SIM_TOL, (what, err)
        assert np.isnan(np.asarray(got_sim)[~got]).all(), what
    counts = np.bincount(got_assign[got], minlength=C)
    assert np.array_equal(np.asarray(got_counts), counts), what
    want_obj = float(mine[got].mean()) if got.any() else 0.0
    print(f"{what}: objective error {abs(float(got_objective) - want_obj):.3g}")
    assert abs(float(got_objective) - want_obj) <= SIM_TOL, (what, float(got_objective), want_obj)
    # cent against the fp64 sum over the kernel's own assignment: 2 (n_c + 4) 2^-24 sum_i |xh_ia| per element -- the first-order bound
    # of any fp32 summation order of n_c terms plus the rounding of xh, doubled; empty clusters keep their input bits
    want = cluster.update_reference(x, got_assign, cent_in)
    got_cent = np.asarray(got_cent)
    empty = counts == 0
    assert np.array_equal(got_cent[empty].view(np.int32), np.asarray(cent_in, dtype=np.float32)[empty].view(np.int32)), what
    worst = 0.0
    for c in np.nonzero(~empty)[0]:
        rows = x[got_assign == c].astype(np.float64)
        xh = rows / np.linalg.norm(rows, axis=1, keepdims=True)
        bound = 2.0 * (counts[c] + 4) * 2.0 ** -24 * np.abs(xh).sum(axis=0)
        err = np.abs(got_cent[c].astype(np.float64) - want[c])
        worst = max(worst, float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()))
        assert (err <= bound).all(), (what, int(c), float(err.max()))
    print(f"{what}: worst centroid error / bound {worst:.3g}")
    return {"excused": int(excused.sum()), "cent": worst}


# ---- whole fits --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_inputs(case):
    N, D, C, a, seed, _ = case
    x, y = feats(seed, N, D, C, a)
    init = x[np.random.default_rng(99 + seed).choice(N, C, replace=False)].copy()
    return _freeze(x, y, init)


@functools.lru_cache(maxsize=None)
def exact_reference(case):
    x, _, init = exact_inputs(case)
    return cluster.kmeans_reference(x, init, case[5] + 4)


def assert_exact_conditions(case):
    ref = exact_reference(case)
    assert ref.info["converged"] == 1 and ref.info["iters_run"] == case[5] >= 5, (case, ref.info)
    assert min(float(g.min()) for g in ref.gaps) >= EXACT_GAP, case


@functools.lru_cache(maxsize=None)
def forced_inputs(case):
    N, D, C, a, _ = case
    x, y = feats(N, N, D, C, a)
    init = x[np.random.default_rng(99).choice(N, C, replace=False)].copy()
    return _freeze(x, y, init)


@functools.lru_cache(maxsize=None)
def forced_reference(case):
    x, _, init = forced_inputs(case)
    return cluster.kmeans_reference(x, init, case[4])


def assert_forced_conditions(case):
    ref = forced_reference(case)
    assert max(float((g < SIM_GAP).mean()) for g in ref.gaps) <= FORCED_SHARE, case


@functools.lru_cache(maxsize=None)
def empty_inputs():
    N, D, C = EMPTY_CASE
    x, y = feats(5, N, D, 10, 1.0)
    cent = np.concatenate([x, np.random.default_rng(6).standard_normal((C - N, D)).astype(np.float32)])
    return _freeze(x, y, cent)


def check_trace_tail(changed, objective, iters_run):
    changed, objective = np.asarray(changed), np.asarray(objective)
    assert (changed[iters_run:] == -1).all() and np.isnan(objective[iters_run:]).all()
    assert (changed[:iters_run] >= 0).all() and np.isfinite(objective[:iters_run]).all()
