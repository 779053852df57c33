"""Inputs and cached fp64 references shared by the t-SNE tests (test_tsne_cpu.py, test_tsne_gpu.py)."""
import functools

import numpy as np

from rspnet_amd import tsne

GATE = 2e-5                    # the project's per-kernel tolerance, relative to the tensor's largest magnitude
KNIFE = 1e-4                   # a coordinate with |g| below this share of max |g| is excluded from the exact gains comparison
MAX_EXCLUDED = 0.02            # ... and at most this share of the coordinates may be
PERPLEXITY, LR, EXAG, EXAG_ITERS, FIT_ITERS = 20.0, 50.0, 12.0, 250, 350
FORCED = (0, 1, 5, 100, 249, 250, 299)


def clusters(seed, groups, per, D, noise):
    """groups x per rows around `groups` random centres, and their labels."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((groups, D))
    y = np.repeat(np.arange(groups), per)
    x = (mu[y] + noise * rng.standard_normal((groups * per, D))).astype(np.float32)
    return x, y.astype(np.int64)


@functools.lru_cache(maxsize=None)
def main_input():
    """The 300-row input of the issue: 6 clusters x 50 rows, D = 32, noise 0.5."""
    x, y = clusters(0, 6, 50, 32, 0.5)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def main_sched():
    s = tsne.schedule(FIT_ITERS, LR, EXAG, EXAG_ITERS)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def main_y0():
    import torch
    y0 = tsne.initial_map(torch.from_numpy(np.array(main_input()[0])), 0, "random").numpy()
    y0.setflags(write=False)
    return y0


@functools.lru_cache(maxsize=None)
def main_reference():
    """The fp64 trajectory of the whole fit on the 300-row input (350 iterations), with the states before the FORCED iterations.
    Computed once, shared, never modified."""
    x, _ = main_input()
    return tsne.tsne_reference(x, PERPLEXITY, main_sched(), main_y0(), FIT_ITERS, keep=FORCED)


def implied_gradient(inc_out, inc_in, gains_out, lr, mom):
    """g from inc' = mom inc - lr gains' g, in fp64."""
    return -(np.asarray(inc_out, np.float64) - mom * np.asarray(inc_in, np.float64)) / (lr * np.asarray(gains_out, np.float64))


def knife_edge(g_ref):
    """The coordinates whose gains sign test is a knife edge, from the reference gradient alone; asserts the cap."""
    ex = np.abs(g_ref) < KNIFE * np.abs(g_ref).max()
    assert ex.mean() <= MAX_EXCLUDED, f"{int(ex.sum())} of {ex.size} coordinates excluded"
    return ex


def expected_gains(g_ref, inc_in, gains_in):
    """The gains update in fp32 with the branch the reference gradient takes: what an exact implementation stores."""
    inc32, gn = np.asarray(inc_in, np.float32), np.asarray(gains_in, np.float32)
    return np.maximum(np.where((g_ref > 0) != (inc32 > 0), gn + np.float32(0.2), gn * np.float32(0.8)), np.float32(0.01))


def close(got, want, what, record=None, scale=None):
    """|got - want| <= GATE * max |want| (or `scale`); prints the figure first."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max()) if scale is None else float(scale)
    err = float(np.abs(got - want).max()) / scale if scale > 0 else float(np.abs(got - want).max())
    print(f"tsne-figure {what}: {err:.3e} (gate {GATE:.0e})")
    if record is not None:
        record.append((what, err))
    assert err <= GATE, (what, err)
    return err
