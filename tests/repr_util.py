"""Shared by the representation-statistics tests: seeded inputs, the fp64 reference computed once per case, the error measures and
their gate."""
import functools

import numpy as np

from rspnet_amd import repr_stats

GATE = 2e-5      # the GPU suite's per-kernel gate


@functools.lru_cache(maxsize=None)
def case_input(N, D, kind="normal"):
    rng = np.random.default_rng(1000 * N + D)
    if kind == "normal":
        x = rng.standard_normal((N, D))
    elif kind == "offset":      # a common direction: the pair sums do not cancel, the Gram matrix has one large eigenvalue
        x = rng.standard_normal((N, D)) + 0.7 * rng.standard_normal((1, D))
    elif kind == "collapsed":
        x = 1.0 + 1e-3 * rng.standard_normal((N, D))
    else:
        raise ValueError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case_reference(N, D, kind="normal", t=2.0):
    return repr_stats.repr_reference(case_input(N, D, kind), t)


def errors(got, ref):
    """pair_exp / pair_cos2: relative error; pair_cos: absolute error per pair (its sum cancels on centred data); gram: error relative
    to max |gram|; colsum: absolute error per valid row (every term is at most 1 in magnitude)."""
    M = int(ref["rows_valid"])
    pairs = max(M * (M - 1) // 2, 1)
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    gmax = max(float(np.abs(ref["gram"]).max()), 1e-300) if M else 1.0
    return {"pair_exp": rel(got["pair_exp"], ref["pair_exp"]) if M >= 2 else abs(got["pair_exp"]),
            "pair_cos2": rel(got["pair_cos2"], ref["pair_cos2"]) if M >= 2 else abs(got["pair_cos2"]),
            "pair_cos": abs(got["pair_cos"] - ref["pair_cos"]) / pairs,
            "gram": float(np.abs(np.asarray(got["gram"]) - ref["gram"]).max()) / gmax,
            "colsum": float(np.abs(np.asarray(got["colsum"]) - ref["colsum"]).max()) / max(M, 1)}


def check(got, ref, what=""):
    """Prints every figure, then asserts the counts and the gate; returns the errors."""
    e = errors(got, ref)
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert (int(got["rows_valid"]), int(got["rows_bad"])) == (int(ref["rows_valid"]), int(ref["rows_bad"])), what
    assert not np.isnan(np.asarray(got["gram"])).any() and not np.isnan(np.asarray(got["colsum"])).any(), what
    for k, v in e.items():
        assert v <= GATE, (what, k, v)
    return e
